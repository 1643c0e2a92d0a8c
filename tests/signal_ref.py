"""
Test infrastructure: the raw-to-chunk-rows path of the reference, restated line by line with its dtypes, plus the case list that
tests/golden/make_golden.py (make_signal_fixture), tests/test_signal_ref_cpu.py and tests/test_gpu_signal.py share.

What is restated (NumPy on the CPU; nothing of bonito_amd is imported):
  bonito/pod5.py:57     scaled = scaling * (raw.astype(np.float32) + offset)          scaling / offset are Python floats -> fp32
  bonito/pod5.py:61     shift, scale = normalisation(scaled, scaling_strategy, norm_params)                  reader.py:142-166
  bonito/pod5.py:62     trimmed = trim(scaled, threshold=scale * 2.4 + shift)   on the pA signal             reader.py:122-139
  bonito/pod5.py:67     signal = (scaled[trimmed:] - shift) / scale             fp32 or fp64, by NumPy's promotion of shift / scale
  bonito/util.py::chunk and `.to(torch.float16)` of bonito/crf/basecall.py:33 (torch rounds fp64 -> fp32 -> fp16)

`shift` / `scale` are np.float64 from np.quantile or Python's own `10` / `1.0` / config floats; which of the two decides the dtype of
everything after (NEP 50): a Python scalar leaves an fp32 array fp32, a np.float64 promotes it to fp64. The threshold
`scale * 2.4 + shift` is a Python float only when both are, and then `scaled > threshold` compares in fp32.

One deviation: the reference's `chunk` divides by zero on an empty signal (a read with nothing left after the trim); `chunk_rows`
returns no rows for it, as the product skips such reads.
"""
import hashlib

import numpy as np
import torch

DEFAULT_NORM_PARAMS = {"quantile_a": 0.2, "quantile_b": 0.9, "shift_multiplier": 0.51, "scale_multiplier": 0.53}


def normalisation(sig, scaling_strategy=None, norm_params=None):
    if scaling_strategy and scaling_strategy.get("strategy") == "pa":
        if norm_params and norm_params.get("standardise") == 1:
            shift = norm_params.get("mean")
            scale = norm_params.get("stdev")
        elif norm_params and norm_params.get("standardise") == 0:
            shift = 0.0
            scale = 1.0
        else:
            raise ValueError("Picoampere scaling requested, but standardisation flag not provided")
    elif scaling_strategy is None or scaling_strategy.get("strategy") == "quantile":
        if norm_params is None:
            norm_params = DEFAULT_NORM_PARAMS
        qa, qb = np.quantile(sig, [norm_params["quantile_a"], norm_params["quantile_b"]])
        shift = max(10, norm_params["shift_multiplier"] * (qa + qb))
        scale = max(1.0, norm_params["scale_multiplier"] * (qb - qa))
    else:
        raise ValueError("unsupported scaling strategy")
    return shift, scale


def above(signal, threshold):
    """The trim predicate, in the reference's form and precision: the pA signal against `scale * 2.4 + shift`."""
    return signal > threshold


def trim(signal, window_size=40, threshold=2.4, min_trim=10, min_elements=3, max_samples=8000, max_trim=0.3):
    seen_peak = False
    num_windows = min(max_samples, len(signal)) // window_size
    for pos in range(num_windows):
        start = pos * window_size + min_trim
        end = start + window_size
        window = signal[start:end]
        if len(window[above(window, threshold)]) > min_elements or seen_peak:
            seen_peak = True
            if above(window[-1], threshold):
                continue
            if end >= min(max_samples, len(signal)) or end / len(signal) > max_trim:
                return min_trim
            return end
    return min_trim


def is_python_scalar(x):
    return not isinstance(x, np.generic)


def ingest(raw, scaling, offset, scaling_strategy=None, norm_params=None, do_trim=True):
    """int16 samples + calibration -> dict(shift, scale, threshold, trim, scaled, signal) as bonito/pod5.py:57-67 leaves them."""
    raw = np.asarray(raw)
    assert raw.dtype == np.int16
    scaled = float(scaling) * (raw.astype(np.float32) + float(offset))
    assert scaled.dtype == np.float32
    shift, scale = normalisation(scaled, scaling_strategy, norm_params)
    threshold = scale * 2.4 + shift
    trimmed = trim(scaled, threshold=threshold) if do_trim else 0
    signal = (scaled[trimmed:] - shift) / scale
    return {"shift": shift, "scale": scale, "threshold": threshold, "trim": int(trimmed), "scaled": scaled, "signal": signal}


def chunk(signal, chunksize, overlap):
    """bonito/util.py::chunk for a 1-D signal, in NumPy: [n, 1, chunksize]."""
    signal = np.asarray(signal)[None, :]
    T = signal.shape[-1]
    if T < chunksize:
        n, overhang = divmod(chunksize, T)
        return np.concatenate((np.tile(signal, n), signal[..., :overhang]), axis=-1)[None, :]
    step = chunksize - overlap
    stub = (T - overlap) % step
    rest = signal[0, stub:]
    rows = [rest[s:s + chunksize] for s in range(0, len(rest) - chunksize + 1, step)]
    if stub > 0:
        rows.insert(0, signal[0, :chunksize])
    return np.stack(rows)[:, None, :]


def to_half(x):
    """`.to(torch.float16)` of basecall.py:33 on the CPU."""
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.float16).numpy()


def chunk_rows(signal, chunksize, overlap):
    """fp16 [n, 1, chunksize] rows of one read (no rows for an empty signal)."""
    if len(signal) == 0:
        return np.zeros((0, 1, chunksize), np.float16)
    return to_half(chunk(signal, chunksize, overlap))


def f64_bits(x):
    return int(np.float64(x).view(np.uint64))


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.blake2b(a.tobytes(), digest_size=8).hexdigest()


# ---- reads by recipe ----------------------------------------------------------------------------------------------------------------------
def make_raw(recipe):
    """int16 samples from a recipe (a JSON-able dict). Steps are applied in this order:
      n, fill: [v0, v1, ...]        the values repeated cyclically over n samples                      (constant, two values, ...)
      runs: [[value, count], ...]   concatenated instead of fill (sorted reads with chosen ranks)
      domain: true                  every int16 value once, ascending
      gauss: [seed, mean, sd, n]    rounded and clipped normal draws
      set: [[start, stop, step, value], ...]   overwrite samples start:stop:step
      shuffle: seed                 a permutation of the whole read
    """
    if "gauss" in recipe:
        seed, mean, sd, n = recipe["gauss"]
        x = np.clip(np.round(np.random.default_rng(seed).normal(mean, sd, n)), -32768, 32767)
    elif "runs" in recipe:
        x = np.concatenate([np.full(c, v) for v, c in recipe["runs"]])
    elif recipe.get("domain"):
        x = np.arange(-32768, 32768)
    else:
        fill = np.asarray(recipe["fill"])
        x = fill[np.arange(recipe["n"]) % len(fill)]
    x = x.astype(np.int16)
    for start, stop, step, value in recipe.get("set", []):
        x[start:stop:step] = value
    if "shuffle" in recipe:
        x = x[np.random.default_rng(recipe["shuffle"]).permutation(len(x))]
    return np.ascontiguousarray(x)


QUANTILE = None
PA_MODEL = ({"strategy": "pa"}, {"standardise": 1, "mean": 93.69239463939118, "stdev": 23.506745239082388})
PA_ROUND = ({"strategy": "pa"}, {"standardise": 1, "mean": 93.7, "stdev": 23.5})
PA_PLAIN = ({"strategy": "pa"}, {"standardise": 0})
Q_EXTREME = ({"strategy": "quantile"}, {"quantile_a": 0.0, "quantile_b": 1.0, "shift_multiplier": 0.51, "scale_multiplier": 0.53})
Q_MEDIAN = ({"strategy": "quantile"}, {"quantile_a": 0.5, "quantile_b": 0.5, "shift_multiplier": 0.51, "scale_multiplier": 0.53})

# a read of two alternating levels (80 / 96 pA at scaling 0.2: shift 89.76, scale 8.48, threshold 110.1 pA = raw 550.6) onto which
# the trim cases write samples of raw 1000; windows are [10 + 40 p, 50 + 40 p)
_BASE = [400, 480]
_LASTS = lambda first, stop: [first, stop, 40, 1000]          # the last sample of consecutive windows


def _case(name, recipe, scaling=0.1755, offset=-243.0, mode=QUANTILE, do_trim=True):
    strategy, params = mode if mode else (None, None)
    return {"name": name, "recipe": recipe, "scaling": scaling, "offset": offset, "strategy": strategy, "params": params,
            "do_trim": do_trim}


def cases():
    out = []
    # lengths: around the trim window (40, +min_trim 10), a wave, the stats block, max_samples 8000, and T = 1, 7, L - 1, L, L + 1
    # after the trim for the chunk lengths below
    for i, n in enumerate([1, 2, 3, 10, 11, 17, 39, 40, 41, 49, 50, 51, 73, 74, 75, 76, 77, 255, 256, 257, 1023, 1030, 1031,
                           8000, 8039, 8040, 8041, 8050, 12000]):
        rec = {"gauss": [100 + i, 480, 60, n]}
        if n >= 255:
            rec["set"] = [[50, 50 + min(n // 8, 170), 1, 900]]
        out.append(_case("len%d" % n, rec))
    for n in (1, 2, 7, 63, 64, 65):
        out.append(_case("len%d_notrim" % n, {"gauss": [200 + n, 480, 60, n]}, do_trim=False))
    # value patterns
    out.append(_case("constant", {"n": 5000, "fill": [517]}))                                    # both weak
    out.append(_case("two_values", {"n": 3001, "fill": [400, 480]}, 0.2, 0.0))
    out.append(_case("tiny_values", {"n": 6000, "fill": [0, 1, 2, 3, 4, 5, 6]}, 0.05, 0.0))      # both weak, not constant
    out.append(_case("weak_shift", {"n": 4000, "fill": [-100, 100, -100, 100, 90]}, 0.2, 0.0))   # shift = 10, scale np.float64
    out.append(_case("weak_scale", {"n": 4000, "fill": [500, 501]}, 0.2, 0.0))                   # scale = 1.0, shift np.float64
    out.append(_case("weak_shift_peak", {"n": 4000, "fill": [-100, 100, -100, 100, 90], "set": [[50, 170, 1, 2000]]}, 0.2, 0.0))
    out.append(_case("weak_scale_peak", {"n": 4000, "fill": [500, 501], "set": [[50, 170, 1, 600]]}, 0.2, 0.0))
    out.append(_case("weak_both_peak", {"n": 4000, "fill": [10], "set": [[50, 170, 1, 100]]}, 0.2, 0.0))
    out.append(_case("extremes", {"gauss": [31, 480, 60, 3000], "set": [[5, 3000, 97, -32768], [9, 3000, 89, 32767]]}))
    out.append(_case("top_bin", {"runs": [[100, 700], [32600, 100], [32767, 200]], "shuffle": 3}))
    out.append(_case("bottom_bin", {"runs": [[-32768, 150], [-32700, 150], [0, 700]], "shuffle": 4}))
    out.append(_case("all_top", {"n": 300, "fill": [32767, 32766, 32512]}, 0.01, 0.0))
    out.append(_case("all_bottom", {"n": 300, "fill": [-32768, -32767, -32513]}, 0.01, 40000.0))
    # ranks on bin boundaries: n = 1000 -> ranks 199 / 200 (gamma 0.8) and 899 / 900 (gamma 0.1)
    out.append(_case("rank_high_byte", {"runs": [[-5, 100], [255, 100], [256, 300], [700, 400], [1024, 100]]}))     # 255 | 256, 767.. | 1024
    out.append(_case("rank_high_byte_shuffled", {"runs": [[-5, 100], [255, 100], [256, 300], [700, 400], [1024, 100]], "shuffle": 5}))
    out.append(_case("rank_low_byte", {"runs": [[520, 200], [521, 300], [600, 400], [601, 100]], "shuffle": 6}))    # inside bins 0x82
    out.append(_case("rank_skips_bins", {"runs": [[-3000, 200], [9000, 700], [20000, 100]], "shuffle": 7}))         # prev | next far apart
    out.append(_case("rank_sorted_12", {"runs": [[100, 1], [200, 1], [511, 1], [512, 1], [600, 5], [767, 1], [768, 1], [800, 1]]},
                     do_trim=False))
    # quantile parameters
    for mode, tag in ((Q_EXTREME, "q01"), (Q_MEDIAN, "q55")):
        out.append(_case("gauss_" + tag, {"gauss": [41, 480, 60, 2500], "set": [[50, 170, 1, 900]]}, mode=mode))
        out.append(_case("extremes_" + tag, {"gauss": [42, 480, 60, 999], "set": [[5, 999, 97, -32768], [9, 999, 89, 32767]]}, mode=mode))
        out.append(_case("len1_" + tag, {"n": 1, "fill": [480]}, mode=mode, do_trim=False))
        out.append(_case("len2_" + tag, {"n": 2, "fill": [480, 520]}, mode=mode, do_trim=False))
    # trim
    out.append(_case("trim_no_peak", {"n": 2000, "fill": _BASE}, 0.2, 0.0))
    out.append(_case("trim_peak_ends", {"n": 2000, "fill": _BASE, "set": [[50, 170, 1, 1000]]}, 0.2, 0.0))                     # 210
    out.append(_case("trim_peak_to_limit", {"n": 12000, "fill": _BASE, "set": [[50, 90, 1, 1000], _LASTS(129, 7970)]}, 0.2, 0.0))
    out.append(_case("trim_peak_past_limit", {"n": 12000, "fill": _BASE, "set": [[50, 90, 1, 1000], _LASTS(129, 8050)]}, 0.2, 0.0))
    out.append(_case("trim_peak_before_limit", {"n": 30000, "fill": _BASE, "set": [[50, 90, 1, 1000], _LASTS(129, 7930)]}, 0.2, 0.0))   # 7970
    out.append(_case("trim_past_max_trim", {"n": 1000, "fill": _BASE, "set": [[50, 90, 1, 1000], _LASTS(129, 370)]}, 0.2, 0.0))
    out.append(_case("trim_below_max_trim", {"n": 1000, "fill": _BASE, "set": [[50, 90, 1, 1000], _LASTS(129, 250)]}, 0.2, 0.0))        # 290
    out.append(_case("trim_at_max_trim", {"n": 1100, "fill": _BASE, "set": [[50, 90, 1, 1000], _LASTS(129, 290)]}, 0.2, 0.0))           # 330 / 1100
    out.append(_case("trim_three_above", {"n": 2000, "fill": _BASE, "set": [[60, 63, 1, 1000]]}, 0.2, 0.0))
    out.append(_case("trim_four_above", {"n": 2000, "fill": _BASE, "set": [[60, 64, 1, 1000]]}, 0.2, 0.0))                     # 90
    out.append(_case("trim_only_last_above", {"n": 2000, "fill": _BASE, "set": [[89, 90, 1, 1000]]}, 0.2, 0.0))
    out.append(_case("trim_last_above_rest_below", {"n": 2000, "fill": _BASE, "set": [[60, 64, 1, 1000], _LASTS(89, 250)]}, 0.2, 0.0))  # 290
    out.append(_case("trim_clipped_window_last_above", {"n": 45, "fill": _BASE, "set": [[20, 24, 1, 1000], [44, 45, 1, 1000]]}, 0.2, 0.0))
    out.append(_case("trim_clipped_window_last_below", {"n": 45, "fill": _BASE, "set": [[20, 24, 1, 1000]]}, 0.2, 0.0))
    out.append(_case("trim_clipped_second_window", {"n": 85, "fill": _BASE, "set": [[20, 24, 1, 1000], [49, 50, 1, 1000], [84, 85, 1, 1000]]},
                     0.2, 0.0))
    # raw 2899 at this calibration is 150.10000610 pA against a threshold of 23.5 * 2.4 + 93.7 = 150.1 -> 150.10000610 in fp32: not above
    # in the reference's form, above as `(scaled - 93.7) / 23.5 > 2.4`; the window holds three more samples above, so the trim tells
    for raw in (2898, 2899, 2900):
        out.append(_case("trim_edge_raw%d" % raw, {"n": 2000, "fill": [1500, 1600], "set": [[60, 63, 1, 5000], [63, 64, 1, raw]]},
                         0.05681302398443222, -257.0, PA_ROUND))
    out.append(_case("trim_off", {"n": 2000, "fill": _BASE, "set": [[50, 170, 1, 1000]]}, 0.2, 0.0, do_trim=False))
    # fixed pA, and the whole int16 domain
    for mode, tag in ((PA_MODEL, "pa_model"), (PA_ROUND, "pa_round"), (PA_PLAIN, "pa_plain")):
        for do_trim in (True, False):
            t = tag + ("" if do_trim else "_notrim")
            out.append(_case("gauss_" + t, {"gauss": [51, 480, 60, 9000], "set": [[50, 170, 1, 1500]]}, 0.2, 10.0, mode, do_trim))
            out.append(_case("domain_" + t, {"domain": True}, 0.2, 10.0, mode, do_trim))
            out.append(_case("domain_shuffled_" + t, {"domain": True, "shuffle": 9}, 0.2, 10.0, mode, do_trim))
    out.append(_case("domain", {"domain": True}, 0.2, 10.0))
    out.append(_case("domain_shuffled", {"domain": True, "shuffle": 9}, 0.2, 10.0))
    out.append(_case("domain_shuffled_small_cal", {"domain": True, "shuffle": 10}, 0.0007, 3.0, PA_PLAIN))   # threshold 2.4f inside the range
    assert len({c["name"] for c in out}) == len(out)
    return out


# (chunk length, overlap, longest read it is applied to): 64..67 and 1021..1027 straddle the kernel's four-samples-per-thread stores
# and its 256-thread block; overlap L - 1 makes one row per sample, so only short reads get it
GEOMETRIES = [(64, 0, None), (65, 7, None), (66, 0, None), (67, 5, None), (1021, 100, None), (1024, 0, None), (1025, 12, None),
              (1027, 500, None), (996, 498, None), (4000, 500, None), (64, 63, 300), (67, 66, 300)]


def geometries_of(n):
    return [(L, ov) for L, ov, longest in GEOMETRIES if longest is None or n <= longest]
