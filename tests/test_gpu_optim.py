"""bonito_amd.optim.AdamW on the device (-m gpu) against tests/optim_ref.py.

Every parameter, gradient and state tensor is a view into a larger buffer whose other elements hold a pattern; the pattern is asserted
untouched after every step. After each of three steps p, m and v must equal, byte for byte, the numpy fp32 restatement evaluated with the
scalars the device left in the control block; the control block itself is checked against the fp64 restatement: step, the beta
products, clip coefficient, gradient multiplier, 1 - beta1^step, the loss scale and the growth tracker exactly (IEEE fp64 multiply,
divide and subtract), the gradient norm within CHUNK * 2^-24 relative (the worst case of an fp32 sum of CHUNK squares; the fp64
additions behind it add nothing visible), and sqrt(1 - beta2^step) within one fp64 rounding."""
import io

import numpy as np
import pytest
import torch

import optim_ref as ref
from bonito_amd import _lib
from bonito_amd.optim import CTL, KERNEL_SCALAR, KERNEL_VECTOR, AdamW

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 64                      # guard elements on either side; keeps a view at offset PAD 16-byte aligned
PATTERN = -7.5
CHUNK = 8192                  # asserted against bh_optim_chunk below
SIZES = [1, 3, 4, 5, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7]
EXACT = ("scale", "growth_tracker", "step", "beta1_pow", "beta2_pow", "clip_coef", "skipped", "scale_used", "grad_mul")


def _guarded(values, shift=0):
    """-> (buffer, view): `values` inside a buffer of PATTERN, the view starting PAD + shift elements in."""
    n = values.numel()
    buf = torch.full((n + 2 * PAD + 4,), PATTERN, dtype=torch.float32, device=DEV)
    view = buf[PAD + shift:PAD + shift + n]
    view.copy_(values)
    return buf, view


def _guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    return bool((buf[:lo] == PATTERN).all()) and bool((buf[lo + view.numel():] == PATTERN).all())


class Rig:
    """Parameters of the given sizes in guarded buffers, an AdamW over them with guarded state, and a host mirror."""

    def __init__(self, sizes, seed=0, p_shift=(), g_shift=(), no_grad=(), frozen=(), groups=None, **opt_kw):
        self.gen = torch.Generator().manual_seed(seed)
        self.sizes, self.g_shift, self.no_grad, self.frozen = list(sizes), set(g_shift), set(no_grad), set(frozen)
        self.buffers, self.params = [], []
        for i, n in enumerate(sizes):
            buf, view = _guarded(torch.randn(n, generator=self.gen), shift=1 if i in p_shift else 0)
            p = torch.nn.Parameter(view, requires_grad=i not in self.frozen)
            self.buffers.append((buf, view))
            self.params.append(p)
        if groups is None:
            self.opt = AdamW(self.params, **opt_kw)
        else:                                      # groups: [(indices, dict of group options)]
            self.opt = AdamW([dict(params=[self.params[i] for i in idx], **kw) for idx, kw in groups], **opt_kw)
        self.active = [i for i in range(len(sizes)) if i not in self.no_grad and i not in self.frozen]
        for i in self.active:
            st = self.opt.state[self.params[i]]
            st["step"] = torch.tensor(0.0)
            for key in ("exp_avg", "exp_avg_sq"):
                buf, view = _guarded(torch.zeros(sizes[i]))
                self.buffers.append((buf, view))
                st[key] = view

    def group_of(self, i):
        return next(g for g in self.opt.param_groups if any(q is self.params[i] for q in g["params"]))

    def new_grads(self, magnitude):
        """Fresh guarded gradients (a new allocation every step, as backward() makes them) -> {index: float32 array}."""
        self.grad_buffers, grads = [], {}
        for i in self.active:
            values = torch.randn(self.sizes[i], generator=self.gen) * magnitude
            buf, view = _guarded(values, shift=1 if i in self.g_shift else 0)
            self.grad_buffers.append((buf, view))
            self.params[i].grad = view
            grads[i] = values.numpy().copy()
        return grads

    def snapshot(self):
        out = {}
        for i in range(len(self.sizes)):
            st = self.opt.state.get(self.params[i], {})
            out[i] = tuple(t.detach().cpu().numpy().copy() if t is not None else None
                           for t in (self.params[i], st.get("exp_avg"), st.get("exp_avg_sq")))
        return out

    def guards_intact(self):
        return all(_guards_intact(b, v) for b, v in self.buffers + self.grad_buffers)

    def checked_step(self, grads, max_norm, use_scale=True):
        """One opt.step() with everything the module docstring promises asserted; -> the control block after it."""
        before, c0 = self.snapshot(), self.opt.control()
        self.opt.step(max_norm=max_norm)
        after, c1 = self.snapshot(), self.opt.control()
        assert self.guards_intact()
        for i in self.active:                                      # g is never written
            assert np.array_equal(self.params[i].grad.cpu().numpy().view(np.int32), grads[i].view(np.int32)), i
        betas = self.opt.param_groups[0]["betas"]
        want = ref.finalise(c0, ref.sum_of_squares(grads.values()), max_norm, use_scale, self.opt.growth_factor, self.opt.backoff_factor,
                            self.opt.growth_interval, betas)
        if not want["skipped"]:
            rel = abs(c1["grad_norm"] - want["grad_norm"]) / want["grad_norm"]
            print("grad_norm %.9g against fp64 %.9g: relative error %.3e (bound %.3e)" % (c1["grad_norm"], want["grad_norm"], rel, CHUNK * 2.0 ** -24))
            assert rel <= CHUNK * 2.0 ** -24
            # the clip coefficient follows from the norm the device found: restate it from that
            clip = min(1.0, max_norm / (c1["grad_norm"] + 1e-6)) if max_norm is not None and max_norm > 0 else 1.0
            want.update(clip_coef=clip, grad_mul=clip / want["scale_used"])
            assert c1["bias1"] == want["bias1"]
            assert abs(c1["bias2_sqrt"] - want["bias2_sqrt"]) <= 2.0 ** -52 * want["bias2_sqrt"]
        for key in EXACT:
            assert c1[key] == want[key], (key, c1[key], want[key])
        for i in range(len(self.sizes)):
            p0, m0, v0 = before[i]
            if i not in self.active:
                assert np.array_equal(after[i][0].view(np.int32), p0.view(np.int32)) and after[i][1] is None, i
                continue
            g = self.group_of(i)
            exp = ref.adamw_fp32(p0, grads[i], m0, v0, c1, g["lr"], g["betas"], g["eps"], g["weight_decay"])
            for name, got, e in zip("pmv", after[i], exp):
                if not np.array_equal(got.view(np.int32), e.view(np.int32)):
                    bad = np.flatnonzero(got.view(np.int32) != e.view(np.int32))
                    raise AssertionError("tensor %d (n=%d) %s: %d elements differ from the fp32 restatement, first at %d: %r against %r, "
                                         "largest distance %d ulp" % (i, self.sizes[i], name, len(bad), bad[0], got[bad[0]], e[bad[0]],
                                                                      ref.ulp_distance(got, e)))
            if not c1["skipped"] and np.abs(grads[i]).max() * abs(c1["grad_mul"]) > 1e-12:
                assert not np.array_equal(after[i][0], p0), "tensor %d did not move" % i
        return c1


def test_chunk_and_control_block_match_the_header():
    assert _lib.lib().bh_optim_chunk() == CHUNK
    assert torch.zeros(1).cuda().data_ptr() % 16 == 0 and (PAD * 4) % 16 == 0


CASES = {
    "clip_inactive": dict(max_norm=1e6, opt=dict(weight_decay=0.01), magnitude=65536.0 * 0.02),
    "clip_active": dict(max_norm=0.1, opt=dict(weight_decay=0.01), magnitude=65536.0 * 0.02),
    "no_max_norm": dict(max_norm=None, opt=dict(weight_decay=0.0), magnitude=65536.0 * 0.02),
    "denormal_square": dict(max_norm=2.0, opt=dict(weight_decay=0.01, loss_scale=None), magnitude=None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_three_steps_write_the_bytes_of_the_fp32_restatement(name):
    case = CASES[name]
    sizes = SIZES + [1031, 2 * CHUNK + 5, 300, 300]
    n = len(SIZES)
    rig = Rig(sizes, seed=1, p_shift={n}, g_shift={n + 1}, no_grad={n + 2}, frozen={n + 3}, lr=2e-3, **case["opt"])
    use_scale = case["opt"].get("loss_scale", 1.0) is not None
    for step in range(3):
        if case["magnitude"] is None:              # every gradient 1e-20: its square, and v, are denormal in fp32
            grads = rig.new_grads(1.0)
            for i in grads:
                grads[i][:] = np.float32(1e-20)
                rig.params[i].grad.fill_(1e-20)
            assert 0 < float(np.float32(1e-3) * np.float32(1e-20) * np.float32(1e-20)) < np.finfo(np.float32).tiny
        else:
            grads = rig.new_grads(case["magnitude"])
        c = rig.checked_step(grads, case["max_norm"], use_scale)
        assert c["step"] == step + 1 and not c["skipped"]
        if name == "clip_active":
            assert c["clip_coef"] < 1.0
        if name == "clip_inactive":
            assert c["clip_coef"] == 1.0
    assert _lib.lib().bh_optim_last_kernel() == KERNEL_VECTOR | KERNEL_SCALAR
    assert rig.params[n + 2] not in rig.opt.state and rig.params[n + 3] not in rig.opt.state


@pytest.mark.parametrize("count", [33, 65])
def test_more_tensors_than_one_launch_holds(count):
    """33 and 65 tensors cross the 32-tensor table once and twice; two larger tensors put several slots on either side of a crossing."""
    sizes = [1 + (7 * i) % 61 for i in range(count)]
    sizes[5], sizes[count - 1] = 2 * CHUNK + 3, CHUNK + 1
    rig = Rig(sizes, seed=count, lr=1e-3, weight_decay=0.01)
    for step in range(3):
        rig.checked_step(rig.new_grads(65536.0 * 0.05), 2.0)
    assert _lib.lib().bh_optim_last_kernel() == KERNEL_VECTOR


def test_two_groups_with_different_lr_and_weight_decay():
    sizes = [257, CHUNK + 1, 5, 3 * CHUNK + 7]
    rig = Rig(sizes, seed=4, groups=[([0, 1], dict(lr=2e-3, weight_decay=0.01)), ([2, 3], dict(lr=5e-4, weight_decay=0.0))])
    assert rig.group_of(0)["lr"] != rig.group_of(3)["lr"]
    for step in range(3):
        rig.checked_step(rig.new_grads(65536.0 * 0.02), 2.0)


@pytest.mark.parametrize("kind", ["inf", "nan", "square_overflows"])
def test_an_overflowed_step_changes_nothing_but_the_loss_scale(kind):
    sizes = [5, 257, CHUNK + 1, 3 * CHUNK + 7]
    rig = Rig(sizes, seed=7, lr=2e-3, growth_interval=2)
    rig.checked_step(rig.new_grads(65536.0 * 0.02), 2.0)           # m, v and the step are not at their initial values
    before, c0 = rig.snapshot(), rig.opt.control()
    grads = rig.new_grads(65536.0 * 0.02)
    bad = {"inf": np.float32("inf"), "nan": np.float32("nan"), "square_overflows": np.float32(3e19)}[kind]
    grads[2][CHUNK - 1] = bad                                       # the last element of the first chunk of the third tensor
    rig.params[2].grad[CHUNK - 1] = float(bad)
    with np.errstate(over="ignore", invalid="ignore"):
        assert np.isfinite(bad) == (kind == "square_overflows") and not np.isfinite(np.float32(bad) * np.float32(bad))
    c1 = rig.checked_step(grads, 2.0)
    after = rig.snapshot()
    for i in range(len(sizes)):
        for a, b in zip(after[i], before[i]):
            assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert all(c1[k] == c0[k] for k in ("step", "beta1_pow", "beta2_pow"))
    assert c1["scale"] == c0["scale"] / 2 and c1["growth_tracker"] == 0 and c1["skipped"] == 1
    grad_norm, scale_used, skipped = rig.opt.last()
    assert skipped and scale_used == c0["scale"] and not np.isfinite(grad_norm)
    for _ in range(2):                                              # growth_interval = 2: two clean steps double the scale
        c2 = rig.checked_step(rig.new_grads(65536.0 * 0.02), 2.0)
    assert c2["scale"] == c1["scale"] * 2 and c2["growth_tracker"] == 0 and not rig.opt.last()[2]


def _run(seed, steps, state=None):
    rig = Rig([5, 257, CHUNK + 1, 2 * CHUNK + 7], seed=seed, p_shift={1}, lr=2e-3)
    for _ in range(steps):
        rig.checked_step(rig.new_grads(65536.0 * 0.02), 1.0)
    return rig


def test_two_runs_from_equal_state_give_equal_bytes():
    a, b = _run(11, 3).snapshot(), _run(11, 3).snapshot()
    for i in a:
        for x, y in zip(a[i], b[i]):
            assert np.array_equal(x.view(np.int32), y.view(np.int32))


def test_a_state_dict_round_trip_continues_with_equal_bytes():
    rig = _run(13, 2)
    saved = rig.opt.state_dict()
    assert [float(s["step"]) for s in saved["state"].values()] == [2.0] * 4
    assert saved["param_groups"][0]["loss_scale"] == 65536.0 and saved["param_groups"][0]["growth_tracker"] == 2
    params = [torch.nn.Parameter(p.detach().clone()) for p in rig.params]
    fresh = AdamW(params, lr=2e-3)
    blob = io.BytesIO()                         # through a file, as optim_N.tar goes: load_state_dict keeps the tensors it is given
    torch.save(saved, blob)
    blob.seek(0)
    fresh.load_state_dict(torch.load(blob, map_location=DEV))
    for k in ("scale", "growth_tracker", "step", "beta1_pow", "beta2_pow"):
        assert fresh.control()[k] == rig.opt.control()[k], k
    grads = rig.new_grads(65536.0 * 0.02)
    for p, i in zip(params, sorted(grads)):
        p.grad = torch.from_numpy(grads[i]).to(DEV)
    rig.checked_step(grads, 1.0)
    fresh.step(max_norm=1.0)
    for p, q in zip(params, rig.params):
        for x, y in ((p, q), (fresh.state[p]["exp_avg"], rig.opt.state[q]["exp_avg"]), (fresh.state[p]["exp_avg_sq"], rig.opt.state[q]["exp_avg_sq"])):
            assert np.array_equal(x.detach().cpu().numpy().view(np.int32), y.detach().cpu().numpy().view(np.int32))
    assert fresh.control() == rig.opt.control()


def test_scale_multiplies_the_loss_without_reading_the_control_block_on_the_host():
    p = torch.nn.Parameter(torch.ones(8, device=DEV))
    opt = AdamW([p], loss_scale=1024.0)
    loss = (p * 0.5).sum()
    scaled = opt.scale(loss)
    assert scaled.dtype == torch.float32 and float(scaled) == 4096.0
    scaled.backward()
    assert bool((p.grad == 512.0).all())
    opt.step(max_norm=None)
    grad_norm, scale, skipped = opt.last()
    assert scale == 1024.0 and not skipped and abs(grad_norm - 0.5 * 8 ** 0.5) < 1e-6
    off = AdamW([p], loss_scale=None)
    assert off.scale(loss) is loss
