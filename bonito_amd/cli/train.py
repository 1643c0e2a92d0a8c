"""
``python -m bonito_amd train``: train a CRF model of the LSTM or the transformer family, or with --norm batch a QuartzNet CTC model, on labelled chunks (chunks.npy, references.npy, reference_lengths.npy,
what ``basecaller --save-ctc`` writes) on one HIP device -- the arguments of the reference's bonito/cli/train.py.

The training directory receives config.toml (the model's config, the arguments under [training]), per epoch weights_N.tar,
losses_N.csv (chunks, time, grad_norm, lr, scale, loss per step) and every --save-optim-every epochs optim_N.tar, and training.csv
(one row per epoch); ``basecaller`` and ``evaluate`` load it. The step is bonito_amd.training.Trainer's: forward_train, the CTC-CRF loss,
backward and bonito_amd.optim.AdamW, all on the device in fp16 with fp32 master weights; --no-amp has nothing to select and is refused.
``--norm batch`` trains a model whose convolutions carry a BatchNorm (every published configuration) with batch statistics.
"""
import os
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser
from importlib import import_module
from pathlib import Path

import torch

from bonito_amd.data import load_data
from bonito_amd.training import Trainer
from bonito_amd.util import _model_dir, dump_toml, init, load_model, load_symbol, load_toml


def _refuse(message):
    print("[error] %s" % message)
    raise SystemExit(1)


def main(args):
    workdir = os.path.expanduser(args.training_directory)
    if os.path.exists(workdir) and not args.force:
        _refuse("%s exists, use -f to force continue training." % workdir)
    os.makedirs(workdir, exist_ok=True)
    if args.no_amp:
        _refuse("--no-amp is not served: forward_train computes in fp16 with fp32 master weights and there is no fp32 path")
    if args.directory is None:
        _refuse("--directory (chunks.npy, references.npy, reference_lengths.npy) is required")
    if not args.pretrained and not args.config:
        _refuse("one of --config and --pretrained is required")
    if args.num_workers:
        print("[--num-workers is ignored: batches are index slices of the arrays, there are no loader processes]")
    if args.nondeterministic:
        print("[--nondeterministic is ignored: the kernels have one order of summation]")

    init(args.seed, args.device)
    device = torch.device(args.device)
    if not args.pretrained:
        config = load_toml(args.config)
    else:
        config = load_toml(os.path.join(_model_dir(args.pretrained), "config.toml"))
        if "lr_scheduler" in config:
            print("[ignoring 'lr_scheduler' in --pretrained config]")
            del config["lr_scheduler"]
    argsdict = {"training": {k: v for k, v in vars(args).items() if k not in ("func", "command", "_argv")}}
    argsdict["training"]["pwd"] = os.getcwd()

    print("[loading model]")
    if args.pretrained:
        print("[using pretrained model %s]" % args.pretrained)
        model = load_model(args.pretrained, device, half=False)
    else:
        model = load_symbol(config, "Model")(config)
    if not hasattr(model, "forward_train"):
        _refuse("%s.%s has no forward_train: the LSTM and transformer families of CRF models and the QuartzNet CTC models train on the device" % (type(model).__module__, type(model).__name__))
    model = model.to(device)

    print("[loading data]")
    train_loader, valid_loader = load_data(args.directory, args.chunks, args.valid_chunks, args.batch, args.seed)
    chunks_per_epoch = args.chunks or len(train_loader.lengths)
    if chunks_per_epoch < args.batch:
        _refuse("%d training chunks are fewer than one batch of %d" % (chunks_per_epoch, args.batch))
    norm_kwargs = {} if args.norm is None else {"norm": args.norm}
    # what forward_train refuses, it refuses in front of its first launch. With --norm batch the probe runs in train mode (load_model
    # returns eval mode) and would rewrite the running statistics: they are put back, byte for byte.
    buffers = {name: b.clone() for name, b in model.named_buffers()} if norm_kwargs else {}
    was_training = model.training
    try:
        if norm_kwargs:
            model.train()
        with torch.no_grad():
            model.forward_train(next(iter(valid_loader))[0][:1].to(torch.float16).to(device), **norm_kwargs)
    except ValueError as exc:
        _refuse(str(exc))
    finally:
        model.train(was_training)
        with torch.no_grad():
            for name, b in model.named_buffers():
                if name in buffers:
                    b.copy_(buffers[name])

    with open(os.path.join(workdir, "config.toml"), "w") as fh:
        dump_toml({**config, **argsdict}, fh)

    lr_scheduler_fn = None
    if config.get("lr_scheduler"):
        sched = dict(config["lr_scheduler"])
        package = {"bonito.schedule": "bonito_amd.schedule"}.get(sched["package"], sched["package"])
        lr_scheduler_fn = getattr(import_module(package), sched["symbol"])(**sched)

    trainer = Trainer(model, device, train_loader, valid_loader, use_amp=True, lr_scheduler_fn=lr_scheduler_fn, restore_optim=args.restore_optim,
                      save_optim_every=args.save_optim_every, grad_accum_split=args.grad_accum_split,
                      quantile_grad_clip=args.quantile_grad_clip, chunks_per_epoch=chunks_per_epoch, batch_size=args.batch, **norm_kwargs)
    lr = [float(x) for x in args.lr.split(",")] if "," in args.lr else float(args.lr)
    trainer.fit(workdir, args.epochs, lr, **config.get("optim", {}))
    return 0


def argparser():
    parser = ArgumentParser(
        formatter_class=ArgumentDefaultsHelpFormatter,
        add_help=False,
        description="Train a CRF model of the LSTM or the transformer family, or with --norm batch a QuartzNet CTC model, on labelled chunks on one HIP device; the training directory receives config.toml, "
                    "weights_N.tar, optim_N.tar, losses_N.csv and training.csv.",
    )
    parser.add_argument("training_directory")
    group = parser.add_mutually_exclusive_group()
    group.add_argument("--config", default=None)
    group.add_argument("--pretrained", default="")
    parser.add_argument("--directory", type=Path)
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--lr", default="2e-3")
    parser.add_argument("--seed", default=25, type=int)
    parser.add_argument("--epochs", default=5, type=int)
    parser.add_argument("--batch", default=64, type=int)
    parser.add_argument("--chunks", default=0, type=int)
    parser.add_argument("--valid-chunks", default=None, type=int)
    parser.add_argument("--no-amp", action="store_true", default=False)
    parser.add_argument("-f", "--force", action="store_true", default=False)
    parser.add_argument("--restore-optim", action="store_true", default=False)
    parser.add_argument("--nondeterministic", action="store_true", default=False)
    parser.add_argument("--save-optim-every", default=10, type=int)
    parser.add_argument("--grad-accum-split", default=1, type=int)
    quantile = parser.add_mutually_exclusive_group()
    quantile.add_argument("--quantile-grad-clip", dest="quantile_grad_clip", action="store_true")
    quantile.add_argument("--no-quantile-grad-clip", dest="quantile_grad_clip", action="store_false")
    quantile.set_defaults(quantile_grad_clip=True)
    parser.add_argument("--num-workers", default=4, type=int)
    parser.add_argument("--norm", default=None, choices=["batch"],
                        help="how a convolution's BatchNorm trains: batch = with batch statistics, updating the running ones; "
                             "without the option a model with norms (every QuartzNet CTC model among them) is refused")
    return parser
