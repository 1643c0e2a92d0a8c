"""
CTC-CRF model surface of the MI355X engine: mirrors ``bonito.crf.model`` (/root/reference
bonito/crf/model.py) -- ``get_stride``, ``CTC_CRF``, ``rnn_encoder``, ``SeqdistModel``, ``Model`` -- with
every koi / cuDNN call replaced by the HIP engine:

* ``Model.use_koi(batchsize, chunksize, quantize)`` (crf/model.py:240-246) == ``use_hip``: the encoder is
  lowered to ``bh_encoder_*`` (built lazily on first forward, i.e. after ``load_state_dict`` / ``half`` /
  ``to`` / ``fuse_bn_`` which the reference loader runs *after* use_koi, util.py:292-310);
* ``CTC_CRF.viterbi / logZ / posteriors`` (crf/model.py:47-67,98-103) call the HIP decode kernels.
"""
import numpy as np
import torch

from bonito_amd import decode as hip_decode
from bonito_amd.engine import EngineHolder, HipEncoder
from bonito_amd.nn import (Module, Convolution, LinearCRFEncoder, Serial, Permute, layers, to_dict, from_dict,
                           register, NoTorchCompute)


def get_stride(m, stride=1):
    """Total down-sampling of a module tree (reference crf/model.py:15-27)."""
    if hasattr(m, "output_stride"):
        return m.output_stride(stride)
    if hasattr(m, "stride"):
        s = m.stride
        if isinstance(s, tuple):
            assert len(s) == 1
            s = s[0]
        return stride * s
    for child in m.children():
        stride = get_stride(child, stride)
    return stride


class _CtcLoss(torch.autograd.Function):
    """CTC_CRF.ctc_loss with a backward: per-chunk loss [N] of device scores. The forward takes logz and the edge posteriors of both
    log-sums from one launch each (bh_crf_seq_logz_grad, bh_crf_logz_dense_grad) and keeps post_dense - post_chain in fp32; the
    backward scales it by upstream * clip_mask / length. The value is computed by the expression of the no-grad path, from the
    same numbers (contiguous koi-layout scores take logZ from bh_crf_logz there, so here too)."""

    @staticmethod
    def forward(ctx, scores, targets, target_lengths, state_len, loss_clip, normalise_scores, blank_score):
        keep = torch.empty(scores.shape, dtype=torch.float32, device=scores.device)
        if normalise_scores:
            lz, _ = hip_decode.logz_grad(scores, state_len, blank_score, out=keep)
            S = 4 ** state_len
            half = scores.detach().to(torch.float16)
            if scores.shape[-1] == 4 * S and (half if half.stride(2) == 1 else half.contiguous()).is_contiguous():
                lz = hip_decode.logz_any(half, state_len, blank_score)              # (bh_crf_logz, as the no-grad path)
            minus = torch.full((scores.shape[1 if scores.shape[-1] == 5 * S else 0],), -1.0, device=scores.device)
            logz, _ = hip_decode.seq_logz_grad(scores, targets, target_lengths, state_len, blank_score, weight=minus, out=keep,
                                               accumulate=True)
            logz = logz.double() - lz.double()
        else:
            logz, _ = hip_decode.seq_logz_grad(scores, targets, target_lengths, state_len, blank_score, out=keep)
            keep.neg_()
            logz = logz.double()
        lengths = target_lengths.to(logz.device)
        loss = (-(logz / lengths)).float()
        scale = torch.isfinite(loss).float() / lengths.float()                  # a target that cannot fit: +inf loss, zero gradient
        if loss_clip:
            scale = scale * ((loss >= 0.0) & (loss <= loss_clip)).float()       # torch.clamp's gradient: 1 inside [0, clip]
            loss = torch.clamp(loss, 0.0, loss_clip)
        ctx.save_for_backward(keep, scale)
        ctx.five = scores.shape[-1] == 5 * 4 ** state_len
        ctx.dtype = scores.dtype
        return loss

    @staticmethod
    def backward(ctx, upstream):
        keep, scale = ctx.saved_tensors
        w = upstream.float() * scale
        grad = keep * (w[None, :, None] if ctx.five else w[:, None, None])
        return grad.to(ctx.dtype), None, None, None, None, None, None


class CTC_CRF:
    """k-mer CTC-CRF sequence distribution (reference crf/model.py:30-108).

    State j is a base-4 k-mer (oldest base most significant). ``idx[j, 0] = j`` (stay) and
    ``idx[j, 1+r] = r*S/4 + j//4`` (move into j having dropped base r)."""

    def __init__(self, state_len, alphabet):
        self.alphabet = alphabet
        self.state_len = state_len
        self.n_base = len(alphabet[1:])
        S = self.n_base ** self.state_len
        states = torch.arange(S)
        self.idx = torch.cat([
            states[:, None],
            states.repeat_interleave(self.n_base).reshape(self.n_base, -1).T,
        ], dim=1).to(torch.int32)

    def n_score(self):
        return len(self.alphabet) * self.n_base ** self.state_len

    def viterbi(self, scores):
        """Best path on expand_blanks-layout scores [T, N, 5*S] (cuda fp16/fp32) -> [T, N] in {0..4}
        (0 = no emission), as reference crf/model.py:98-103."""
        moves, path = hip_decode.viterbi_5s(scores.to(torch.float16), self.state_len)
        return path.T.to(torch.int64)

    def path_to_str(self, path):
        alphabet = np.frombuffer("".join(self.alphabet).encode(), dtype="u1")
        seq = alphabet[path[path != 0]]
        return seq.tobytes().decode()

    def reverse_complement(self, scores):
        """Permute scores so that decoding yields the reverse-complement strand (reference crf/model.py:84-96).
        Accepts the engine's koi layout [N, T, 4S] or the reference layout [T, N, 5S] (cuda fp16)."""
        S = self.n_base ** self.state_len
        if scores.shape[-1] == 4 * S:
            return hip_decode.reverse_complement(scores.contiguous())
        return hip_decode.reverse_complement_5s(scores, self.state_len)

    def logZ(self, scores, blank_score=2.0):
        """Log partition function per chunk of koi-layout scores [N, T, 4S] (reference crf/model.py:47-52)."""
        return hip_decode.logz(scores.contiguous(), blank_score)

    def posteriors(self, scores, blank_score=None):
        """Edge posteriors of the Log semiring (the reference's SequenceDist.posteriors: the gradient of logZ), for the reference
        layout [T, N, 5S] or the engine layout [N, T, 4S] with ``blank_score`` (the four move edges per state; the stay edge
        is a scalar there). Shape and dtype of ``scores``. The Max semiring stays with ``viterbi`` / ``posterior_viterbi``."""
        return hip_decode.logz_grad(scores, self.state_len, blank_score)[1]

    def normalise(self, scores):
        """scores - logZ / T on the reference layout [T, N, 5S] (reference crf/model.py:54-55). The koi layout keeps its stay
        score outside the tensor, so it cannot be normalised in place; ``ctc_loss`` never needs the normalised copy."""
        if scores.shape[-1] != self.n_score():
            raise ValueError("normalise needs the reference layout [T, N, %d]" % self.n_score())
        logz = hip_decode.logz_any(scores, self.state_len).to(scores.dtype)
        return scores - logz[:, None] / len(scores)

    def prepare_ctc_scores(self, scores, targets):
        """The plain torch gather of the reference (crf/model.py:110-124), kept for API parity and for tests: the HIP scans gather
        the same edges inside the kernel and never build these [T, N, L] tensors."""
        targets = torch.clamp(targets - 1, 0)
        T, N, C = scores.shape
        scores = scores.to(torch.float32)
        n = targets.size(1) - (self.state_len - 1)
        stay_indices = sum(
            targets[:, i:n + i] * self.n_base ** (self.state_len - i - 1)
            for i in range(self.state_len)
        ) * len(self.alphabet)
        move_indices = stay_indices[:, 1:] + targets[:, :n - 1] + 1
        stay_scores = scores.gather(2, stay_indices.expand(T, -1, -1))
        move_scores = scores.gather(2, move_indices.expand(T, -1, -1))
        return stay_scores, move_scores

    def ctc_loss(self, scores, targets, target_lengths, loss_clip=None, reduction="mean", normalise_scores=True,
                 blank_score=None):
        """-ln P(target | scores) / target_length per chunk (reference crf/model.py:126-139).
        scores: the reference layout [T, N, 5S], or the engine layout [N, T, 4S] with ``blank_score``; cuda fp16 (fp32 is
        rounded to fp16). With ``normalise_scores`` no normalised copy is written: normalisation subtracts logZ / T from each
        of the T edges of every path, so the loss is -(seq_logz(raw) - logZ(raw)) / target_length.
        Device scores with ``requires_grad`` are differentiable: d loss_n / d scores = clip_mask_n / length_n * (posteriors of
        logZ - posteriors of the target chain), from the alpha-beta kernels of csrc/seqdist_grad.hip, in the dtype and layout of
        ``scores``; the values equal the no-grad path's bit for bit. fp32 scores are rounded to fp16 for the kernels and the
        gradient is that of the ROUNDED scores, passed straight through. A chunk whose target cannot fit into T steps has loss
        +inf and a zero gradient; a clipped chunk (loss outside [0, loss_clip]) has a zero gradient, as with torch.clamp.
        Host tensors with requires_grad are refused (NoTorchCompute): there is no torch compute path."""
        if reduction not in ("mean", "none", None):
            raise ValueError("Unknown reduction type {}".format(reduction))
        if scores.requires_grad and torch.is_grad_enabled():
            if not scores.is_cuda:
                raise NoTorchCompute("ctc_loss has a backward on a HIP device only: host scores with requires_grad are refused")
            hip_decode.seq_layout(scores, self.state_len, blank_score)
            loss = _CtcLoss.apply(scores, targets, target_lengths, self.state_len, loss_clip, bool(normalise_scores), blank_score)
            return loss.mean() if reduction == "mean" else loss
        logz = hip_decode.seq_logz(scores, targets, target_lengths, self.state_len, blank_score).double()
        if normalise_scores:
            logz = logz - hip_decode.logz_any(scores, self.state_len, blank_score)
        loss = (-(logz / target_lengths.to(logz.device))).float()
        if loss_clip:
            loss = torch.clamp(loss, 0.0, loss_clip)
        return loss.mean() if reduction == "mean" else loss

    def ctc_viterbi_alignments(self, scores, targets, target_lengths, blank_score=None):
        """Forced alignment (reference crf/model.py:141-143) -> int32 [N, T] on the CPU: the chain position (index of the
        target's k-mer) occupied after every step; see ``bonito_amd.decode.seq_viterbi`` for the definition."""
        return hip_decode.seq_viterbi(scores, targets, target_lengths, self.state_len, blank_score)[0]


def conv(c_in, c_out, ks, stride=1, bias=False, activation=None, norm=None):
    return Convolution(c_in, c_out, ks, stride=stride, padding=ks // 2, bias=bias, activation=activation, norm=norm)


def rnn_encoder(n_base, state_len, insize=1, first_conv_size=4, stride=5, winlen=19, activation="swish",
                rnn_type="lstm", features=768, scale=5.0, blank_score=None, expand_blanks=True, num_layers=5,
                norm=None):
    """Old-style ([encoder] without `type`) conv x3 -> alternating LSTMs -> tanh*scale CRF head
    (reference crf/model.py:150-162)."""
    rnn = layers[rnn_type]
    return Serial([
        conv(insize, first_conv_size, ks=5, bias=True, activation=activation, norm=norm),
        conv(first_conv_size, 16, ks=5, bias=True, activation=activation, norm=norm),
        conv(16, features, ks=winlen, stride=stride, bias=True, activation=activation, norm=norm),
        Permute([2, 0, 1]),
        *(rnn(features, features, reverse=(num_layers - i) % 2) for i in range(num_layers)),
        LinearCRFEncoder(features, n_base, state_len, activation="tanh", scale=scale, blank_score=blank_score,
                         expand_blanks=expand_blanks),
    ])


@register
class SeqdistModel(EngineHolder, Module):
    def __init__(self, encoder, seqdist, n_pre_post_context_bases=None, target_projection=None):
        super().__init__()
        self.seqdist = seqdist
        self.encoder = encoder
        self.stride = get_stride(encoder)
        self.alphabet = seqdist.alphabet
        if n_pre_post_context_bases is None:
            self.n_pre_context_bases = self.seqdist.state_len - 1
            self.n_post_context_bases = 1
        else:
            self.n_pre_context_bases, self.n_post_context_bases = n_pre_post_context_bases
        if target_projection is None:
            self.target_projection = None
        else:
            self.register_buffer("target_projection", torch.tensor([0] + target_projection), persistent=False)

    @classmethod
    def from_dict(cls, model_dict, layer_types=None):
        kwargs = dict(model_dict, encoder=from_dict(model_dict["encoder"], layer_types),
                      seqdist=CTC_CRF(**model_dict["seqdist"]))
        return cls(**kwargs)

    def _lowering(self):
        return self.encoder, dict(quantize=getattr(self, "_quantize", False))

    def engine_replica(self, x):
        """A second, independent engine over the same weights (own workspace): the basecaller keeps `lanes` batches in flight,
        one engine each (crf/basecall.py). Built for the geometry of the model's own engine."""
        eng = self._engine(x)
        return HipEncoder(self.encoder, eng.max_batch, eng.max_chunk, device=eng.device, quantize=getattr(self, "_quantize", False))

    def forward(self, x, *args):
        """x: cuda fp16 [N,1,L] -> scores fp16 [N, T, 4^(state_len+1)] (koi layout, contiguous)."""
        if not x.is_cuda:
            raise NoTorchCompute("bonito_amd models only run on a HIP device; got a %s tensor" % x.device)
        return self._engine(x)(x)

    def _train_plan(self, x, norm):
        """The one walk over the flattened encoder, in front of forward_train's first launch and first side effect: every refusal, and
        -> the steps to run (bonito_amd._train), each with its folding decisions made: the zero channels that pad a convolution pair to a
        multiple of 8, the clamp fused into the layer in front of it, the time-major store in front of the LSTM stack, the BatchNorm step
        behind a normalised convolution and its real channels, batch_major_out of the head, the upsample's view. What is wrong on any
        device is judged first (structure, shapes, parameter dtypes), then ``norm``, then a CPU x, then parameters on another device."""
        from bonito_amd import attn, nn as bnn, rnn, train_ops
        from bonito_amd._train import batchnorm_step, clamp_after, next_compute, pad_channels
        from bonito_amd.engine import _flatten
        from bonito_amd.transformer.model import TransformerEncoderLayer
        mods = _flatten(self.encoder)
        steps = []
        layout = "signal"                        # [N][L] -> "nlc" [N][L][C] -> "tnc" [T][N][C] -> "ntc" scores
        time_major, width = False, None          # has a Permute([2,0,1]) been seen, and how many channels are here (None: not followed)
        length = x.shape[2]                      # positions per chunk behind the convolutions so far
        pad_in = 0                               # zero channels the convolution in front added to its output
        for i, m in enumerate(mods):
            name = "layer %d (%s)" % (i, type(m).__name__)
            if isinstance(m, TransformerEncoderLayer):
                attn.encoder_layer_check(m, "forward_train: %s" % name)
                if time_major:
                    raise ValueError("forward_train: %s follows the permute to time-major activations; a transformer layer needs "
                                     "[N][T][C] (permute [0,2,1])" % name)
                if width is not None and width != m.self_attn.d_model:
                    raise ValueError("forward_train: %s has d_model %d and follows %d channels" % (name, m.self_attn.d_model, width))
                if layout != "nlc":
                    raise ValueError("forward_train: %s needs the [N][T][C] output of the convolutions" % name)
                steps.append(lambda h, seed, m=m: attn.encoder_layer(m, h))
            elif isinstance(m, bnn.LinearUpsample) and not time_major:
                if not m.batch_first:
                    raise ValueError("forward_train: %s with batch_first=False has no training forward" % name)
                if m.d_model % 8 != 0 or (width is not None and width != m.d_model):
                    raise ValueError("forward_train: %s needs d_model %% 8 == 0 and as many input channels (d_model %d, %s channels)"
                                     % (name, m.d_model, width))
                if layout != "nlc":
                    raise ValueError("forward_train: %s needs [N][T][C] activations" % name)
                steps.append(lambda h, seed, m=m: train_ops.linear(h, m.linear.weight, m.linear.bias)      # [N][T][s D], which is [N][s T][D]
                             .view(h.shape[0], h.shape[1] * m.scale_factor, m.d_model))
            elif isinstance(m, bnn.Convolution):
                c, clamp = m.conv, clamp_after(mods, i)
                nxt, tm = next_compute(mods, i)
                pad_out = -c.out_channels % 8 if isinstance(nxt, bnn.Convolution) else 0      # zero channels up to a multiple of 8
                width = c.out_channels
                if m.norm is not None and norm is None:
                    raise ValueError("forward_train: %s carries a norm (%s); a normalised convolution has no training backward yet"
                                     % (name, getattr(m.norm, "name", type(m.norm).__name__)))
                if c.groups != 1 or c.dilation[0] != 1:
                    raise ValueError("forward_train: %s is a grouped / dilated (depthwise, QuartzNet) convolution, which has no training "
                                     "backward" % name)
                if layout not in ("signal", "nlc"):
                    raise ValueError("forward_train: %s follows the permute to time-major activations" % name)
                if (c.in_channels == 1) != (layout == "signal"):
                    raise ValueError("forward_train: %s expects %d input channels" % (name, c.in_channels))
                length = train_ops.conv_out_len(length, c.kernel_size[0], c.stride[0], c.padding[0])
                if m.norm is not None:
                    norm_name = getattr(m.norm, "name", type(m.norm).__name__)
                    if norm != "batch":
                        raise ValueError("forward_train: %s carries a norm (%s) and norm=%r is not served (None, or \"batch\" for batch "
                                         "statistics)" % (name, norm_name, norm))
                    if not isinstance(m.norm, bnn.BatchNorm):
                        raise ValueError("forward_train: %s carries a norm (%s) that is no BatchNorm; norm=\"batch\" serves batchnorm only"
                                         % (name, norm_name))
                    if not m.norm.bn.training:
                        raise ValueError("forward_train: %s has its BatchNorm in eval mode; norm=\"batch\" trains with batch statistics "
                                         "(call model.train()), frozen statistics are not built" % name)
                    if m.norm.bn.track_running_stats and m.norm.bn.momentum is None:
                        raise ValueError("forward_train: %s has a BatchNorm with momentum=None (the cumulative average), which is not "
                                         "served" % name)
                    if (c.out_channels % 8 and not pad_out) or c.out_channels > 2048:
                        raise ValueError("forward_train: %s normalises %d channels; a multiple of 8 up to 2048 is served (zero padding "
                                         "only in front of another convolution)" % (name, c.out_channels))
                    if x.shape[0] * length < 2:
                        raise ValueError("forward_train: %s normalises %d value per channel; batch statistics need more than one"
                                         % (name, x.shape[0] * max(length, 0)))
                if pad_out and clamp is not None and not clamp[0] <= 0.0 <= clamp[1]:
                    raise ValueError("forward_train: %s has %d channels, served by zero padding, and its clamp range %s does not contain 0"
                                     % (name, c.out_channels, clamp))
                # a convolution, a transformer layer or an upsample behind the permute refuses itself, by its own name
                if tm and (nxt is None or isinstance(nxt, (bnn.Linear, bnn.LinearCRFEncoder))):
                    raise ValueError("forward_train: %s stores time-major for a layer that is no LSTM" % name)
                # a normalised convolution is z = conv(x) as it is; norm, activation, clamp and the store are the BatchNorm step's
                steps.append(lambda h, seed, c=c, pads=(pad_in, pad_out), args=(m.activation, clamp, tm) if m.norm is None else (None, None, False):
                             train_ops.conv1d(h, *pad_channels(c.weight, c.bias, *pads), c.stride[0], c.padding[0], *args))
                if m.norm is not None:
                    steps.append(batchnorm_step(m.norm.bn, m.activation, clamp, tm, channels=c.out_channels,
                                                pad=pad_out if m.norm.bn.affine else 0))
                layout, pad_in = "tnc" if tm else "nlc", pad_out
            elif isinstance(m, bnn.LSTM):
                r = m.rnn
                if r.num_layers != 1 or r.bidirectional or r.input_size != r.hidden_size or getattr(r, "proj_size", 0) \
                        or not rnn.supported_hidden_size(r.hidden_size):
                    raise ValueError("forward_train: %s is not an LSTM the device layer serves (one layer, one direction, insize == size, "
                                     "a multiple of 32 in 32..1024)" % name)
                if layout != "tnc":
                    raise ValueError("forward_train: %s must follow permute [2,0,1]" % name)
                steps.append(lambda h, seed, m=m: rnn.lstm_module(m, h))
            elif isinstance(m, bnn.Permute):            # folded: into the store of the convolution in front, or a no-op
                if list(m.dims) not in ([2, 0, 1], [0, 2, 1], [1, 0, 2]):
                    raise ValueError("forward_train: %s with dims %s cannot be folded" % (name, list(m.dims)))
                time_major = time_major or list(m.dims) == [2, 0, 1]
            elif isinstance(m, (bnn.LinearCRFEncoder, bnn.Linear)):
                if layout not in ("tnc", "nlc"):
                    raise ValueError("forward_train: %s needs the time-major output of the LSTM stack or [N][T][C] activations" % name)
                # batch-major rows ([N][T][C], the transformer family) are stored as they are: that is the scores' layout already
                if isinstance(m, bnn.LinearCRFEncoder):
                    args = (m.activation, m.scale if m.scale else None, clamp_after(mods, i), layout == "tnc")
                    layout = "ntc"
                else:
                    args = (None, None, clamp_after(mods, i), False)
                    width = m.linear.out_features
                steps.append(lambda h, seed, m=m, args=args: train_ops.linear(h, m.linear.weight, m.linear.bias, *args))
            elif isinstance(m, bnn.Clamp):
                if i == 0 or not isinstance(mods[i - 1], (bnn.Convolution, bnn.Linear, bnn.LinearCRFEncoder)):
                    raise ValueError("forward_train: %s follows no convolution, linear or head to be fused into" % name)
            elif not isinstance(m, bnn.MakeContiguous):
                raise ValueError("forward_train: %s has no training forward (the LSTM and transformer families of CRF models are served: "
                                 "convolutions, LSTMs, transformer encoder layers, linear, batch-major linearupsample, linearcrfencoder, "
                                 "clamp)" % name)
            for pname, p in m.named_parameters():
                if p.dtype != torch.float32:
                    raise ValueError("forward_train: %s holds %s parameters (%s); training needs the fp32 master weights - call "
                                     "model.float()" % (name, str(p.dtype).replace("torch.", ""), pname))
        if layout != "ntc":
            raise ValueError("forward_train: the encoder does not end in a linearcrfencoder")
        if norm not in (None, "batch"):
            raise ValueError("forward_train: norm=%r is not served (None, or \"batch\" for batch statistics)" % (norm,))
        if not x.is_cuda:
            raise NoTorchCompute("forward_train runs on a HIP device only; x is a %s tensor" % x.device)
        for i, m in enumerate(mods):
            for pname, p in m.named_parameters():
                if p.device != x.device:
                    raise ValueError("forward_train: layer %d (%s) has %s on %s, x is on %s" % (i, type(m).__name__, pname, p.device, x.device))
        return steps

    def forward_train(self, x, norm=None):
        """The forward of a training step: x cuda fp16 [N,1,L] -> scores in the shape, layout and dtype of ``forward(x)``, INSIDE
        autograd, so that ``self.loss(self.forward_train(x), targets, lengths).backward()`` leaves a gradient on every trainable
        parameter. The parameters are the fp32 master weights on x's device; every layer rounds them to fp16 on the device in every
        call (autocast's arithmetic: bonito_amd.train_ops, bonito_amd.rnn, bonito_amd.attn). Serves the LSTM family - conv x3 ->
        permute -> LSTM x n -> [linear] -> linearcrfencoder [-> clamp] - and the transformer family - conv x n (no norm) ->
        permute [0,2,1] -> TransformerEncoderLayer x depth -> LinearUpsample -> linearcrfencoder [-> clamp] - with the folding rules of
        ``engine.lower``: a Clamp after a Convolution or the head is fused into it, Permute([2,0,1]) is folded into the producing
        convolution's store, Permute([0,2,1]) is the layout the convolutions store anyway, Permute([1,0,2]) after the head is a no-op
        (batch-major rows are the scores' layout already), a batch-first LinearUpsample is a linear layer whose [N][T][s D] output is
        read as [N][s T][D]. Anything else is refused with a ValueError that names the layer, and every refusal comes before the first
        launch: ``_train_plan`` judges the whole encoder and returns the steps, which are then only applied. The inference engine is
        neither built nor dropped.

        ``norm`` says what a Convolution that carries a norm gets. None: it is refused. ``"batch"``: a ``bonito_amd.nn.BatchNorm`` in
        train mode normalises with the statistics of this batch, as the reference's training does (conv with no activation ->
        ``train_ops.batchnorm`` with the layer's activation, the fused clamp and the time-major store) - and every call that is not
        refused REWRITES the module's ``running_mean`` / ``running_var`` buffers and adds one to ``num_batches_tracked``, under
        ``torch.no_grad()`` too; a refused call has no side effect. The inference engine holds the statistics of the moment it was
        built: drop it (``_drop_engine``) before inference is to see the new ones. A BatchNorm in eval mode (frozen statistics) is refused."""
        from bonito_amd._train import run
        if getattr(self, "_quantize", False):
            raise ValueError("forward_train: quantize (the 8-bit recurrent path) has no training forward; call use_hip(quantize=False)")
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float16 or x.dim() != 3 or x.shape[1] != 1:
            raise ValueError("forward_train: x must be a float16 tensor [N,1,L], got %s"
                             % ("%s %s" % (x.dtype, tuple(x.shape)) if isinstance(x, torch.Tensor) else type(x).__name__))
        return run(self._train_plan(x, norm), x.reshape(x.shape[0], x.shape[2]))       # [N][L]: one input channel

    def decode_batch(self, x, blank_score=2.0):
        """Posterior decoding of engine scores [N, T, 4S] (cuda fp16) -> list of strings
        (reference crf/model.py:196-199: viterbi over log(posteriors + 1e-8))."""
        _, paths = hip_decode.posterior_viterbi(x.contiguous(), blank_score)
        return [self.seqdist.path_to_str(p) for p in paths.numpy()]

    def decode(self, x):
        return self.decode_batch(x.unsqueeze(0))[0]

    def head_blank_score(self):
        """The fixed stay score of the CRF head (``LinearCRFEncoder.blank_score``), or None for a learned blank column."""
        for m in self.encoder.modules():
            if isinstance(m, LinearCRFEncoder):
                return m.blank_score
        return None

    def loss(self, scores, targets, target_lengths, **kwargs):
        """CTC-CRF loss of labelled chunks (reference crf/model.py:204-207); differentiable for device scores that require
        grad (see ``CTC_CRF.ctc_loss``). ``scores``: this model's engine output [N, T, 4S] (the head's blank score is filled
        in) or the reference layout [T, N, 5S]."""
        if self.target_projection is not None:
            targets = self.target_projection.to(targets.device)[targets.long()]
        if scores.shape[-1] != self.seqdist.n_score():
            kwargs.setdefault("blank_score", self.head_blank_score())
        return self.seqdist.ctc_loss(scores, targets, target_lengths, **kwargs)

    def seq_logprob(self, scores, sequences, blank_score=None):
        """ln P(sequence | scores) per chunk of engine scores [N, T, 4S] -> CPU float64 [N]; ``sequences``: strings or a decoder's
        int8 sequence plane. See ``bonito_amd.decode.seq_logprob``."""
        if blank_score is None:
            blank_score = self.head_blank_score()
        return hip_decode.seq_logprob(scores, sequences, 2.0 if blank_score is None else blank_score)

    def to_dict(self, include_weights=False):
        if include_weights:
            raise NotImplementedError
        res = {
            "encoder": to_dict(self.encoder),
            "seqdist": {"state_len": self.seqdist.state_len, "alphabet": self.seqdist.alphabet},
            "n_pre_post_context_bases": (self.n_pre_context_bases, self.n_post_context_bases),
        }
        if self.target_projection is not None:
            res["target_projection"] = self.target_projection.tolist()[1:]
        return res


class Model(SeqdistModel):
    """``config.toml`` -> model (reference crf/model.py:225-238)."""

    def __init__(self, config):
        seqdist = CTC_CRF(state_len=config["global_norm"]["state_len"], alphabet=config["labels"]["labels"])
        if "type" in config["encoder"]:   # new-style config
            encoder = from_dict(config["encoder"])
        else:                             # old-style
            encoder = rnn_encoder(seqdist.n_base, seqdist.state_len, insize=config["input"]["features"],
                                  **config["encoder"])
        super().__init__(encoder, seqdist,
                         n_pre_post_context_bases=config["input"].get("n_pre_post_context_bases"))
        self.config = config
