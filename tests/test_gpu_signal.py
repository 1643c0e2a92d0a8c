"""Device signal ingest (csrc/signal.hip), bit for bit (-m gpu).

The sweep holds the two kernels to tests/signal_ref.py, the reference's raw-to-chunk-rows path restated line by line, which
tests/test_signal_ref_cpu.py pins to the reference itself (tests/golden/signal_cases.npz) and to bonito_amd/reader.py. Every
comparison is equality of bits: shift and scale as fp64 patterns, the `weak` word they imply, trim, every fp16 chunk sample, and the
guard bytes around the output rows. The reads: signal_ref.cases(); the chunk lengths: signal_ref.GEOMETRIES.

The tests further down compare with the host reader on reads shaped like real ones, and end to end through the basecaller."""
import json

import numpy as np
import pytest
import torch

import signal_ref
from bonito_amd import reader, signal
from bonito_amd.util import chunk

pytestmark = pytest.mark.gpu


# ---- the sweep against the restatement ------------------------------------------------------------------------------------------------------
GUARD = 4096          # bytes of 0xA5 on either side of the output rows


class Group:
    """The cases that share normalisation parameters: one RawBatch, one bh_signal_normalise launch."""

    def __init__(self, cases):
        self.cases = cases
        self.raws = [signal_ref.make_raw(c["recipe"]) for c in cases]
        self.want = [signal_ref.ingest(raw, c["scaling"], c["offset"], c["strategy"], c["params"], c["do_trim"])
                     for raw, c in zip(self.raws, cases)]
        self.batch = signal.RawBatch(self.raws, [c["scaling"] for c in cases], [c["offset"] for c in cases])
        self.shift, self.scale, self.trim = self.batch.normalise(cases[0]["strategy"], cases[0]["params"], do_trim=cases[0]["do_trim"])
        self.weak = self.batch.weak.cpu().numpy()
        self.rows = {}

    def want_rows(self, L, ov, keep):
        """Rows of the restatement for the reads in `keep`, read by read (computed once per geometry)."""
        key = (L, ov, tuple(keep))
        if key not in self.rows:
            self.rows[key] = np.concatenate([np.zeros((0, 1, L), np.float16)] + [
                signal_ref.chunk_rows(w["signal"], L, ov) for w, k in zip(self.want, keep) if k])
        return self.rows[key]

    def table(self, L, ov, keep):
        reads, starts, avail = self.batch.chunk_table(L, ov)
        sel = np.asarray(keep)[reads] if len(reads) else np.zeros(0, bool)
        return reads[sel], starts[sel], avail[sel]


@pytest.fixture(scope="module")
def sweep():
    groups = {}
    for c in signal_ref.cases():
        groups.setdefault(json.dumps([c["strategy"], c["params"], c["do_trim"]], sort_keys=True), []).append(c)
    return [Group(cs) for cs in groups.values()]


def guarded_chunks(batch, table, L, lo=0, hi=None):
    """batch.chunks into a buffer with GUARD bytes of 0xA5 before and behind; -> the rows as uint16 bits on the host."""
    n = len(table[0][lo:hi])
    buf = torch.full((2 * GUARD + 2 * n * L,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[GUARD:GUARD + 2 * n * L].view(torch.float16).view(n, 1, L)
    batch.chunks(table, L, lo, hi, out=out)
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + 2 * n * L:] == 0xA5).all(), "wrote outside the rows"
    return host[GUARD:GUARD + 2 * n * L].view(np.uint16).reshape(n, 1, L)


def test_sweep_shift_scale_weak_trim_equal_restatement(sweep):
    seen = set()
    for g in sweep:
        for i, (c, w) in enumerate(zip(g.cases, g.want)):
            name = c["name"]
            assert int(g.shift[i].view(np.uint64)) == signal_ref.f64_bits(w["shift"]), (name, g.shift[i], w["shift"])
            assert int(g.scale[i].view(np.uint64)) == signal_ref.f64_bits(w["scale"]), (name, g.scale[i], w["scale"])
            fixed = bool(c["strategy"]) and c["strategy"]["strategy"] == "pa"
            weak = 4 if fixed else int(signal_ref.is_python_scalar(w["shift"])) | int(signal_ref.is_python_scalar(w["scale"])) << 1
            assert g.weak[i] == weak, (name, g.weak[i], weak)
            assert g.trim[i] == w["trim"], (name, g.trim[i], w["trim"])
            seen.add(weak)
    assert seen == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("L,ov,longest", signal_ref.GEOMETRIES)
def test_sweep_chunk_rows_equal_restatement(sweep, L, ov, longest):
    """Every fp16 sample of every chunk row: both store paths of the kernel (L % 4), one and two blocks per row, stub chunks, exact
    fits, short reads tiled (T = 1, 7, L - 1 among them), overlap 0 and L - 1."""
    rows = 0
    for g in sweep:
        keep = [longest is None or len(raw) <= longest for raw in g.raws]
        want = g.want_rows(L, ov, keep).view(np.uint16)
        got = guarded_chunks(g.batch, g.table(L, ov, keep), L)
        assert got.shape == want.shape, (g.cases[0]["name"], got.shape, want.shape)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (g.cases[0]["name"], len(bad), bad[:4].tolist())
        rows += len(want)
    assert rows > 0


@pytest.mark.parametrize("L,ov", [(67, 5), (1024, 0)])
def test_sweep_table_slice_starts_inside_a_read(sweep, L, ov):
    for g in sweep:
        keep = [True] * len(g.raws)
        table = g.table(L, ov, keep)
        want = g.want_rows(L, ov, keep).view(np.uint16)
        reads = table[0]
        inside = [k for k in range(1, len(reads)) if reads[k] == reads[k - 1]]       # rows that are not the first of their read
        if not inside:
            continue
        lo = inside[len(inside) // 2]
        hi = min(len(reads), lo + 37)
        assert np.array_equal(guarded_chunks(g.batch, table, L, lo, hi), want[lo:hi]), (g.cases[0]["name"], lo, hi)
        assert guarded_chunks(g.batch, table, L, lo, lo).shape == (0, 1, L)


# ---- against the host reader, on reads shaped like real ones ---------------------------------------------------------------------------------
def _raw_read(rng, n, peak):
    """int16 ADC samples shaped like a nanopore read: an open-pore / adapter stretch, then the read proper."""
    x = rng.normal(480, 60, n)
    if peak and n > 600:
        a = int(rng.integers(20, 200))
        b = a + int(rng.integers(80, 400))
        x[a:b] += rng.normal(420, 30, b - a)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def _cases():
    rng = np.random.default_rng(17)
    raws = [_raw_read(rng, int(n), peak) for n, peak in
            [(50000, True), (12345, True), (9000, False), (3000, True), (700, True), (45, False), (100000, True), (4001, False)]]
    raws.append(np.full(5000, 517, np.int16))                            # constant: scale falls back to the literal 1.0
    raws.append((np.arange(6000) % 7).astype(np.int16))                  # tiny values: shift falls back to the literal 10
    scal = [0.1755, 0.2, 0.15, 0.1755, 0.18, 0.1755, 0.21, 0.1755, 0.1755, 0.05]
    offs = [-243.0, 10.0, -200.0, 3.0, 0.0, -243.0, -100.0, 12.0, -243.0, 0.0]
    return raws, scal, offs


def test_device_normalisation_and_trim_equal_reader():
    raws, scal, offs = _cases()
    batch = signal.RawBatch(raws, scal, offs)
    shift, scale, trim = batch.normalise()
    for i, (raw, sc, of) in enumerate(zip(raws, scal, offs)):
        rd = reader.Read("r%d" % i, raw, scaling=sc, offset=of)
        assert float(rd.shift) == shift[i], (i, rd.shift, shift[i])
        assert float(rd.scale) == scale[i], (i, rd.scale, scale[i])
        assert rd.trimmed_samples == trim[i], (i, rd.trimmed_samples, trim[i])


@pytest.mark.parametrize("chunksize,overlap", [(4000, 500), (996, 498)])
def test_device_chunks_equal_reader_chunk_cast(chunksize, overlap):
    raws, scal, offs = _cases()
    batch = signal.RawBatch(raws, scal, offs)
    batch.normalise()
    table = batch.chunk_table(chunksize, overlap)
    got = batch.chunks(table, chunksize).cpu()
    want = []
    for i, (raw, sc, of) in enumerate(zip(raws, scal, offs)):
        rd = reader.Read("r%d" % i, raw, scaling=sc, offset=of)
        if len(rd.signal):
            want.append(chunk(torch.from_numpy(rd.signal), chunksize, overlap).to(torch.float16))
    want = torch.cat(want)
    assert got.shape == want.shape
    assert torch.equal(got, want)


def test_device_fixed_pa_strategy_and_no_trim():
    raws, scal, offs = _cases()
    batch = signal.RawBatch(raws[:4], scal[:4], offs[:4])
    strat, prm = {"strategy": "pa"}, {"standardise": 1, "mean": 91.25, "stdev": 22.5}
    shift, scale, trim = batch.normalise(strat, prm, do_trim=False)
    assert (shift == 91.25).all() and (scale == 22.5).all() and (trim == 0).all()
    table = batch.chunk_table(2000, 100)
    got = batch.chunks(table, 2000).cpu()
    want = torch.cat([chunk(torch.from_numpy(reader.Read("r", raw, scaling=sc, offset=of, do_trim=False, scaling_strategy=strat,
                                                         norm_params=prm).signal), 2000, 100).to(torch.float16)
                      for raw, sc, of in zip(raws[:4], scal[:4], offs[:4])])
    assert torch.equal(got, want)


def test_basecall_raw_equals_basecall_on_reader_reads():
    """End to end: raw int16 reads through the device ingest give the same calls as reader.Read + the host chunking path."""
    from bonito_amd import synthetic
    from bonito_amd.crf import basecall
    from bonito_amd.crf.basecall import basecall_raw

    class Raw:
        def __init__(self, i, raw, scaling, offset):
            self.read_id, self.raw, self.scaling, self.offset = "read_%d" % i, raw, scaling, offset

    raws, scal, offs = _cases()
    model = synthetic.make_model("fast", batchsize=16, chunksize=3996)
    model.use_koi(batchsize=16, chunksize=3996, quantize=False)
    model = model.half().cuda()
    host_reads = [reader.Read("read_%d" % i, r, scaling=s, offset=o) for i, (r, s, o) in enumerate(zip(raws, scal, offs))]
    want = {rd.read_id: res for rd, res in basecall(model, host_reads, chunksize=3996, overlap=498, batchsize=16)}
    raw_reads = [Raw(i, r, s, o) for i, (r, s, o) in enumerate(zip(raws, scal, offs))]
    got = {rd.read_id: (rd, res) for rd, res in basecall_raw(model, raw_reads, chunksize=3996, overlap=498, batchsize=16)}
    assert set(got) == set(want)
    for hr in host_reads:
        rd, res = got[hr.read_id]
        assert rd.trimmed_samples == hr.trimmed_samples and rd.shift == float(hr.shift) and rd.scale == float(hr.scale)
        assert res["sequence"] == want[hr.read_id]["sequence"]
        assert res["qstring"] == want[hr.read_id]["qstring"]
        assert np.array_equal(res["moves"], want[hr.read_id]["moves"])
