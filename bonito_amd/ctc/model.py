"""
QuartzNet CTC model surface (legacy dna_r9.4.1 `bonito.ctc`) on the MI355X engine: mirrors
/root/reference bonito/ctc/model.py -- ``Model`` (14-57), ``Encoder`` (59-87), ``TCSConv1d`` (90-121),
``Block`` (124-192), ``Decoder`` (195-207) -- as parameter containers with identical module nesting, hence
identical ``state_dict()`` keys (``encoder.encoder.<i>.conv.<j>.{depthwise,pointwise,conv}.weight``,
``...residual.0.conv.weight``, ``decoder.layers.0.{weight,bias}``) and identical seeded initialisation.

``model(x)`` runs the HIP engine (depthwise conv kernel, MFMA pointwise GEMMs with folded BatchNorm and the
residual add fused, 1x1 decoder + log_softmax) and returns log-probabilities in the reference's TNC layout.
The CPU Rust decoders of fast_ctc_decode (:11,39-46) are replaced by bonito_amd.ctc.decode (HIP), and
``torch.nn.functional.ctc_loss`` behind ``ctc_label_smoothing_loss`` / ``loss`` (:48-57) by csrc/ctc_loss.hip.

``model.forward_train(x, norm="batch")`` is the same network inside autograd, layer by layer on the device (bonito_amd.train_ops:
depthwise and pointwise convolution, batch-statistics BatchNorm, residual add with activation and dropout, decoder with log-softmax),
so that ``model.loss(model.forward_train(x, norm="batch"), targets, lengths)["total_loss"].backward()`` leaves a gradient on every
parameter.
"""
import torch
from torch.nn import BatchNorm1d, Conv1d, Dropout, Module, ModuleList, Sequential

from bonito_amd.engine import EngineHolder, lower_ctc
from bonito_amd.nn import NoTorchCompute, Permute, _no_forward, layers


class _CtcLoss(torch.autograd.Function):
    """(nll_n / max(len_n, 1) [N], sum_n smooth_n) of device log_probs with the backward: ONE launch per group of chunks computes the
    values and d loss_n / d log_probs = -occ / max(len_n, 1), kept in fp32; the backward scales it by the upstream gradient of every
    chunk and adds upstream x weights[c] for the smoothing sum. Chunks with an infinite loss get a zero gradient."""

    @staticmethod
    def forward(ctx, log_probs, targets, lengths, weights):
        from bonito_amd import decode
        lens = lengths.to(device=log_probs.device, dtype=torch.float32).clamp(min=1)
        inv = 1.0 / lens
        occ = torch.empty(log_probs.shape, dtype=torch.float32, device=log_probs.device)
        nll, smooth, occ = decode.ctc_nll_grad(log_probs, targets, lengths, weights, weight=inv, out=occ, layout="TNC")
        ctx.save_for_backward(occ, torch.isfinite(nll), torch.as_tensor(weights, dtype=torch.float32).to(log_probs.device))
        ctx.dtype = log_probs.dtype
        return nll / lens, smooth.sum()                                     # (the expression of the no-grad path, bit for bit)

    @staticmethod
    def backward(ctx, g_loss, g_smooth):
        occ, finite, weights = ctx.saved_tensors
        g = occ * g_loss.to(torch.float32)[None, :, None]
        g = g + finite.to(torch.float32)[None, :, None] * (g_smooth.to(torch.float32) * weights)[None, None, :]
        return g.to(ctx.dtype), None, None, None


class TCSConv1d(Module):
    """Time-channel separable 1-D convolution: depthwise (groups=C) + pointwise, or a plain convolution."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=False,
                 separable=False):
        super().__init__()
        self.separable = separable
        if separable:
            self.depthwise = Conv1d(in_channels, in_channels, kernel_size=kernel_size, stride=stride, padding=padding,
                                    dilation=dilation, bias=bias, groups=in_channels)
            self.pointwise = Conv1d(in_channels, out_channels, kernel_size=1, stride=1, dilation=dilation, bias=bias,
                                    padding=0)
        else:
            self.conv = Conv1d(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=padding,
                               dilation=dilation, bias=bias)

    forward = _no_forward


class Block(Module):
    """`repeat` x (TCSConv1d, BatchNorm(eps=1e-3)) with activation/dropout in between, optional pointwise
    residual branch added before the final activation."""

    def __init__(self, in_channels, out_channels, activation, repeat=5, kernel_size=1, stride=1, dilation=1,
                 dropout=0.0, residual=False, separable=False):
        super().__init__()
        self.use_res = residual
        self.conv = ModuleList()
        if stride[0] > 1 and dilation[0] > 1:
            raise ValueError("Dilation and stride can not both be greater than 1")
        padding = (kernel_size[0] // 2) * dilation[0]
        cin = in_channels
        for _ in range(repeat - 1):
            self.conv.extend(self._tcs(cin, out_channels, kernel_size, stride, dilation, padding, separable))
            self.conv.extend((activation, Dropout(p=dropout)))
            cin = out_channels
        self.conv.extend(self._tcs(cin, out_channels, kernel_size, stride, dilation, padding, separable))
        if self.use_res:
            self.residual = Sequential(*self._tcs(in_channels, out_channels))
        self.activation = Sequential(activation, Dropout(p=dropout))

    @staticmethod
    def _tcs(cin, cout, kernel_size=1, stride=1, dilation=1, padding=0, separable=False):
        return [TCSConv1d(cin, cout, kernel_size, stride=stride, dilation=dilation, padding=padding, bias=False,
                          separable=separable),
                BatchNorm1d(cout, eps=1e-3, momentum=0.1)]

    forward = _no_forward


class Encoder(Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        features = config["input"]["features"]
        activation = layers[config["encoder"]["activation"]]()
        blocks = []
        for layer in config["block"]:
            blocks.append(Block(features, layer["filters"], activation, repeat=layer["repeat"],
                                kernel_size=layer["kernel"], stride=layer["stride"], dilation=layer["dilation"],
                                dropout=layer["dropout"], residual=layer["residual"], separable=layer["separable"]))
            features = layer["filters"]
        self.encoder = Sequential(*blocks)

    forward = _no_forward


class Decoder(Module):
    def __init__(self, features, classes):
        super().__init__()
        self.layers = Sequential(Conv1d(features, classes, kernel_size=1, bias=True), Permute([2, 0, 1]))

    forward = _no_forward


class Model(EngineHolder, Module):
    """QuartzNet-style CTC model (https://arxiv.org/abs/1910.10261) from a ``[[block]]`` config."""

    def __init__(self, config):
        super().__init__()
        qs = config.get("qscore")
        self.qbias = qs["bias"] if qs else 0.0
        self.qscale = qs["scale"] if qs else 1.0
        self.config = config
        self.stride = config["block"][0]["stride"][0]
        self.alphabet = config["labels"]["labels"]
        self.features = config["block"][-1]["filters"]
        self.encoder = Encoder(config)
        self.decoder = Decoder(self.features, len(self.alphabet))

    def _lowering(self):
        return self, dict(lowering=lower_ctc)

    def forward(self, x):
        """x: cuda fp16 [N,1,L] -> log-probabilities fp16 [T, N, n_labels] (reference layout, a view)."""
        if not x.is_cuda:
            raise NoTorchCompute("bonito_amd models only run on a HIP device; got a %s tensor" % x.device)
        return self._engine(x)(x).permute(1, 0, 2)

    def _train_plan(self, x):
        """Every check of forward_train about the model, in front of its first launch and its first side effect, and -> the steps to run
        (bonito_amd._train), each with its decisions made: the separable, plain or wide convolution, the BatchNorm step behind it with the
        activation it fuses, and the dropout sites in model order. A block that ends in a residual add or a dropout is one step."""
        from bonito_amd import _lib, train_ops
        from bonito_amd._train import batchnorm_step, pad_channels, run, unsupported_shape
        what = "forward_train"
        N, L, C = int(x.shape[0]), int(x.shape[2]), 1
        plan, sites = [], 0

        def tcs_check(name, tcs, bn, Lin, Cin):
            """-> (the steps of the convolution in front of bn, Lout, Cout)"""
            convs = [("depthwise", tcs.depthwise), ("pointwise", tcs.pointwise)] if tcs.separable else [("conv", tcs.conv)]
            for cname, c in convs:
                if c.dilation[0] != 1:
                    raise ValueError("%s: %s.%s has dilation %d; only dilation 1 has a training backward" % (what, name, cname, c.dilation[0]))
                for pname, t in (("weight", c.weight), ("bias", c.bias)):
                    if t is not None and t.dtype != torch.float32:
                        raise ValueError("%s: %s.%s holds %s parameters (%s); training needs the fp32 master weights"
                                         % (what, name, cname, t.dtype, pname))
            if convs[0][1].in_channels != Cin:
                raise ValueError("%s: %s expects %d input channels and follows %d" % (what, name, convs[0][1].in_channels, Cin))
            Cout = convs[-1][1].out_channels
            if Cout % 8 != 0 or (Cin != 1 and Cin % 8 != 0):
                raise ValueError("%s: %s has %d -> %d channels; multiples of 8 are served" % (what, name, Cin, Cout))
            if tcs.separable:
                dw, pw = tcs.depthwise, tcs.pointwise
                K, pad = dw.kernel_size[0], dw.padding[0]
                if dw.stride[0] != 1 or K > 127:
                    raise ValueError("%s: %s is a separable convolution with stride %d and K = %d; stride 1 and K <= 127 are served"
                                     % (what, name, dw.stride[0], K))
                if Cin % 8 != 0 or dw.groups != Cin or dw.bias is not None or pw.bias is not None:
                    raise ValueError("%s: %s is not a bias-free depthwise + pointwise pair over a multiple of 8 channels" % (what, name))
                train_ops._dw_check(torch.empty((N, Lin, Cin), dtype=torch.float16, device="meta"), dw.weight, pad,
                                    "%s: %s.depthwise" % (what, name), devices=False)
                Lout = train_ops.conv_out_len(Lin, K, 1, pad)
                steps = [lambda h, seed: train_ops.depthwise_conv1d(h, dw.weight, pad),
                         lambda h, seed: train_ops.linear(h, pw.weight[:, :, 0])]
            else:
                c = tcs.conv
                wide = Cin == 1 and Cout > 256          # the single-channel kernel serves 256 filters: seven zero channels ride beside the signal
                shape = (N, Lin) if Cin == 1 and not wide else (N, Lin, 8 if wide else Cin)
                weight = torch.empty((Cout, 8, c.kernel_size[0]), dtype=c.weight.dtype, device="meta") if wide else c.weight
                train_ops._conv_check(torch.empty(shape, dtype=torch.float16, device="meta"), weight, c.bias, c.stride[0], c.padding[0], None,
                                      None, "%s: %s.conv" % (what, name), devices=False)
                if _lib.lib().bh_conv1d_train_workspace(N, Lin, 8 if wide else Cin, Cout, c.kernel_size[0], c.stride[0], c.padding[0]) == 0:
                    raise unsupported_shape("%s: %s.conv" % (what, name), N=N, Lin=Lin, Cin=Cin, Cout=Cout, K=c.kernel_size[0],
                                            stride=c.stride[0], padding=c.padding[0])
                Lout = train_ops.conv_out_len(Lin, c.kernel_size[0], c.stride[0], c.padding[0])
                if wide:
                    steps = [lambda h, seed: train_ops.conv1d(torch.nn.functional.pad(h.unsqueeze(-1), (0, 7)),
                                                              pad_channels(c.weight, None, 7, 0)[0], c.bias, c.stride[0], c.padding[0])]
                else:
                    steps = [lambda h, seed: train_ops.conv1d(h, c.weight, c.bias, c.stride[0], c.padding[0])]
            if not isinstance(bn, BatchNorm1d) or bn.num_features != Cout:
                raise ValueError("%s: %s is not followed by a BatchNorm1d over its %d channels" % (what, name, Cout))
            if not bn.training:
                raise ValueError("%s: %s has its BatchNorm in eval mode; norm=\"batch\" trains with batch statistics (call model.train())"
                                 % (what, name))
            if bn.track_running_stats and bn.momentum is None:
                raise ValueError("%s: %s has a BatchNorm with momentum=None (the cumulative average), which is not served" % (what, name))
            for pname, t in bn.named_parameters():
                if t.dtype != torch.float32:
                    raise ValueError("%s: %s holds %s parameters (BatchNorm %s); training needs the fp32 master weights"
                                     % (what, name, t.dtype, pname))
            if Cout > 2048 or N * Lout < 2:
                raise ValueError("%s: %s normalises %d channels over %d values; up to 2048 channels and more than one value are served"
                                 % (what, name, Cout, N * Lout))
            return steps, Lout, Cout

        def dropped(drop):
            nonlocal sites
            sites += 1
            return (drop.p if drop.training else 0.0), sites - 1

        for bi, block in enumerate(self.encoder.encoder):
            bname = "encoder.encoder.%d" % bi
            mods = list(block.conv)
            convs, i = [], 0            # per TCSConv1d: (its steps, its BatchNorm1d, the Dropout behind its activation or None)
            Lb, Cb = L, C
            while i < len(mods):
                if not isinstance(mods[i], TCSConv1d) or i + 1 >= len(mods):
                    raise ValueError("%s: %s.conv.%d (%s) is no TCSConv1d followed by a BatchNorm1d" % (what, bname, i, type(mods[i]).__name__))
                steps, Lb, Cb = tcs_check("%s.conv.%d" % (bname, i), mods[i], mods[i + 1], Lb, Cb)
                drop = None
                if i + 2 < len(mods):
                    if i + 3 >= len(mods) or not isinstance(mods[i + 3], Dropout):
                        raise ValueError("%s: %s.conv.%d is not followed by an activation and a Dropout" % (what, bname, i + 1))
                    train_ops._act(mods[i + 2], (None, "none", "swish", "tanh", "relu"), "%s: %s" % (what, bname))
                    drop = mods[i + 3]
                convs.append((steps, mods[i + 1], drop))
                i += 4
            act, drop = block.activation[0], block.activation[1]
            train_ops._act(act, (None, "none", "swish", "tanh", "relu"), "%s: %s" % (what, bname))
            for d in [c[2] for c in convs[:-1]] + [drop]:
                if not isinstance(d, Dropout) or not 0.0 <= d.p < 1.0:
                    raise ValueError("%s: %s has a dropout probability outside 0 <= p < 1" % (what, bname))
            res = None
            if block.use_res:
                steps, Lr, Cr = tcs_check("%s.residual" % bname, block.residual[0], block.residual[1], L, C)
                if (Lr, Cr) != (Lb, Cb):
                    raise ValueError("%s: %s adds a residual of %d steps x %d channels to %d x %d" % (what, bname, Lr, Cr, Lb, Cb))
                res = steps + [batchnorm_step(block.residual[1], None)]
            main = []
            for steps, bn, between in convs[:-1]:
                main += steps + [batchnorm_step(bn, act)]
                p, sid = dropped(between)
                if p > 0.0:
                    main.append(lambda h, seed, p=p, sid=sid: train_ops.residual_act(h, None, "none", p, seed, sid))
            p, sid = dropped(drop)
            fused = res is None and p == 0.0        # nothing but the activation follows the last BatchNorm, which fuses it
            main += convs[-1][0] + [batchnorm_step(convs[-1][1], act if fused else None)]
            plan += main if fused else [lambda h, seed, main=main, res=res, act=act, p=p, sid=sid: train_ops.residual_act(
                run(main, h, seed), None if res is None else run(res, h, seed), act, p, seed, sid)]
            L, C = Lb, Cb
        head = self.decoder.layers[0]
        train_ops._head_check(torch.empty((N, L, C), dtype=torch.float16, device="meta"), head.weight, head.bias, "%s: decoder" % what,
                              devices=False)
        plan.append(lambda h, seed: train_ops.ctc_head(h, head.weight, head.bias))
        if not x.is_cuda:
            raise NoTorchCompute("forward_train runs on a HIP device only; x is a %s tensor" % x.device)
        for pname, t in list(self.named_parameters()) + list(self.named_buffers()):
            if t.device != x.device:
                raise ValueError("forward_train: %s is on %s, x is on %s" % (pname, t.device, x.device))
        return plan

    def forward_train(self, x, norm=None, seed=None):
        """x: cuda fp16 [N,1,L] -> log-probabilities fp16 [T, N, n_labels] (the layout of ``forward``, a view of batch-major rows),
        inside autograd: every layer is a device layer of bonito_amd.train_ops with its own backward.

        ``norm`` must be ``"batch"``: every block carries a BatchNorm, which normalises with the statistics of this batch and updates
        its running statistics and ``num_batches_tracked``, as the reference's training does. ``norm=None`` is refused, like every
        other refusal (eval-mode BatchNorm, dilation, a separable convolution with a stride or K > 127, channel counts that are no
        multiples of 8, parameters that are not fp32, what train_ops.conv1d refuses in a plain convolution - K > 32, which is
        dna_r9.4.1@v1's first layer) in front of the first launch and the first side effect: ``_train_plan`` judges the whole model
        and returns the steps, which are then only applied. A single-channel first convolution with more than 256 filters
        (dna_r9.4.1@v2: 344) gets seven zero channels beside the signal, which is what that layer serves.

        Dropout is not stored: site i of the model (every Dropout module, in model order) keeps an element iff a counter-based hash
        of (seed, i, element index) reaches p 2^32 (include/bonito_hip.h). ``seed``: one 64-bit number per call; None draws it from
        torch's default CPU generator - after the plan, so a refused call draws nothing - and torch.manual_seed reproduces a run. A
        Dropout module in eval mode drops nothing."""
        from bonito_amd._train import run
        if norm is None:
            raise ValueError("forward_train: a bonito.ctc model has no forward_train without batch statistics: every block carries a "
                             "BatchNorm; pass norm=\"batch\" / --norm batch")
        if norm != "batch":
            raise ValueError("forward_train: norm=%r is not served (\"batch\" for batch statistics)" % (norm,))
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float16 or x.dim() != 3 or x.shape[1] != 1 or x.shape[0] < 1:
            raise ValueError("forward_train: x must be a float16 tensor [N,1,L], got %s"
                             % ("%s %s" % (x.dtype, tuple(x.shape)) if isinstance(x, torch.Tensor) else type(x).__name__))
        plan = self._train_plan(x)
        if seed is None:
            seed = int(torch.randint(-(1 << 63), (1 << 63) - 1, (1,), dtype=torch.int64).item())
        return run(plan, x[:, 0, :].contiguous(), int(seed) & ((1 << 64) - 1)).permute(1, 0, 2)

    def decode(self, x, beamsize=5, threshold=1e-3, qscores=False, return_path=False):
        """x: log-probabilities [T, n_labels] of ONE read (any device). Greedy when beamsize == 1 or
        qscores (returns seq+qstring concatenated, like fast_ctc_decode.viterbi_search), else prefix beam."""
        from bonito_amd.ctc import decode as ctc_decode
        if beamsize == 1 or qscores:
            seq, path = ctc_decode.viterbi_search(x, self.alphabet, qscores, self.qscale, self.qbias)
        else:
            seq, path = ctc_decode.beam_search(x, self.alphabet, beamsize, threshold)
        return (seq, path) if return_path else seq

    def ctc_label_smoothing_loss(self, log_probs, targets, lengths, weights=None, *, reduction="mean"):
        """The reference's dict {'total_loss', 'loss', 'label_smooth_loss'} (ctc/model.py:48-54) from the device kernel
        (csrc/ctc_loss.hip): loss = mean over n of nll_n / max(len_n, 1) (ctc_loss(reduction='mean')), label_smooth_loss =
        -sum(log_probs * weights) / (T N C), default weights [0.4, 0.1 / (C - 1), ...]. log_probs: device fp16 / fp32 [T, N, C]
        (fp32 is read natively, fp16 is widened in the kernel as the reference's .to(float32) does). reduction='none' puts the
        per-chunk nll_n / max(len_n, 1) into 'loss' (and loss + label_smooth_loss per chunk into 'total_loss').
        With requires_grad the result is differentiable (one launch computes the values and the posterior state occupancies; the
        backward is a scale of them plus the weights[c] / (T N C) term). The kernel's gradient is the TRUE derivative with respect
        to log_probs; torch's native ctc_loss backward returns exp(log_probs) - occ, which is the same thing after log_softmax's
        backward. A chunk whose target cannot fit has an infinite loss and a ZERO gradient (torch: NaN)."""
        if reduction not in ("mean", "none"):
            raise ValueError("reduction must be 'mean' or 'none'")
        if log_probs.requires_grad and not log_probs.is_cuda:
            raise NoTorchCompute("bonito_amd differentiates the CTC loss on a HIP device only; got a %s tensor with requires_grad"
                                 % log_probs.device)
        if log_probs.dim() != 3:
            raise ValueError("log_probs must be [T, N, C], got shape %s" % (tuple(log_probs.shape),))
        from bonito_amd import decode
        T, N, C = log_probs.shape
        if weights is None:
            weights = torch.cat([torch.tensor([0.4]), (0.1 / (C - 1)) * torch.ones(C - 1)])
        weights = torch.as_tensor(weights, dtype=torch.float32)
        if log_probs.requires_grad:
            per_chunk, smooth = _CtcLoss.apply(log_probs, targets, lengths, weights)
        else:
            nll, smooth = decode.ctc_nll(log_probs, targets, lengths, weights, layout="TNC")
            per_chunk = nll / lengths.to(device=nll.device, dtype=torch.float32).clamp(min=1)
            smooth = smooth.sum()
        loss = per_chunk.mean() if reduction == "mean" else per_chunk
        label_smoothing_loss = -smooth / float(T * N * C)
        return {"total_loss": loss + label_smoothing_loss, "loss": loss, "label_smooth_loss": label_smoothing_loss}

    def loss(self, log_probs, targets, lengths, *, reduction="mean"):
        return self.ctc_label_smoothing_loss(log_probs, targets, lengths, reduction=reduction)
