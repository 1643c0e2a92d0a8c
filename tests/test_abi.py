"""The C-ABI library loads and exports every symbol include/bonito_hip.h declares (no GPU calls)."""
import os
import pytest
import re

from conftest import ROOT
from bonito_amd import _lib


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "bonito_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    names = _declared_symbols()
    assert len(names) >= 15
    handle = _lib.lib()
    for n in names:
        assert hasattr(handle, n), "libbonito_hip.so does not export %s" % n
        assert n in _lib.SIGNATURES, "bonito_amd/_lib.py has no ctypes signature for %s" % n
    assert sorted(_lib.SIGNATURES) == names


def test_abi_version_and_error_string():
    handle = _lib.lib()
    assert handle.bh_abi_version() == 1
    assert isinstance(_lib.last_error(), str)


def test_layer_struct_size_matches_header():
    import ctypes
    assert ctypes.sizeof(_lib.bh_layer_t) == _lib.lib().bh_sizeof_layer() == 168


def test_host_packers_run_without_gpu():
    import ctypes as C
    import numpy as np
    handle = _lib.lib()
    H = 32
    w = np.arange(4 * H * H, dtype=np.float32).reshape(4 * H, H) / 1024.0
    out = np.zeros(4 * H * H, np.uint16)
    assert handle.bh_lstm_pack_whh(w.ctypes.data_as(C.c_void_p), H, out.ctypes.data_as(C.c_void_p)) == 0
    halves = out.view(np.float16)
    # slice 1, gate 2, kstep 0, lane 5 (row 5, kgroup 0), j=3  -> W[2H + 16 + 5][3]
    pos = (((1 * 4 + 2) * 1 + 0) * 64 + 5) * 8 + 3
    assert halves[pos] == np.float16(w[2 * H + 16 + 5, 3])
    # lane 21 = row 5, kgroup 1 -> column 8 + j
    pos = (((1 * 4 + 2) * 1 + 0) * 64 + 21) * 8 + 3
    assert halves[pos] == np.float16(w[2 * H + 16 + 5, 11])
    n = handle.bh_conv1d_packed_halves(16, 20, 19)
    assert n == 32 * 320
    cw = np.random.default_rng(0).standard_normal((20, 16, 19)).astype(np.float32)
    pk = np.zeros(n, np.uint16)
    assert handle.bh_conv1d_pack(cw.ctypes.data_as(C.c_void_p), 16, 20, 19, pk.ctypes.data_as(C.c_void_p)) == 0
    pkh = pk.view(np.float16).reshape(32, 320)
    assert pkh[7, 3 * 16 + 5] == np.float16(cw[7, 5, 3])
    assert (pkh[20:] == 0).all() and (pkh[:, 304:] == 0).all()
    assert handle.bh_lstm_pack_whh(w.ctypes.data_as(C.c_void_p), 33, out.ctypes.data_as(C.c_void_p)) != 0
    assert "multiple of 32" in _lib.last_error()


def test_generated_gemm_stream_matches_its_generator(tmp_path):
    """bonito_amd/csrc/gemm_ktile_mfma.inc (one K-tile of gemm_w4_kernel as one instruction stream, with and without the previous
    tile's parked stores) is what tools/gen_gemmstep.py writes with its defaults."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "gemm_ktile_mfma.inc"
    subprocess.run([sys.executable, os.path.join(root, "tools", "gen_gemmstep.py"), "--out", str(out)], check=True, capture_output=True)
    committed = open(os.path.join(root, "bonito_amd", "csrc", "gemm_ktile_mfma.inc")).read()
    assert out.read_text() == committed
    # 64 MFMAs, 32 fragment reads, 16 DMA pieces and exactly one barrier per K-tile function
    body = committed.split("__device__ __forceinline__ void gemm_ktile(")[1].split("__device__ __forceinline__ void")[0]
    assert body.count("v_mfma_f32_32x32x16_f16") == 64 and body.count("ds_read_b128") == 32
    assert body.count("global_load_lds_dwordx4") == 16 and body.count("s_barrier") == 1
    # the same K-tile on 16x16x32 MFMAs (--tile16): 128 MFMAs, the same reads / pieces / barrier; every function one asm statement
    out16 = tmp_path / "gemm_ktile16_mfma.inc"
    subprocess.run([sys.executable, os.path.join(root, "tools", "gen_gemmstep.py"), "--tile16", "--out", str(out16)], check=True, capture_output=True)
    committed = open(os.path.join(root, "bonito_amd", "csrc", "gemm_ktile16_mfma.inc")).read()
    assert out16.read_text() == committed
    body = committed.split("__device__ __forceinline__ void gemm_ktile16(")[1].split("__device__ __forceinline__ void")[0]
    assert body.count("v_mfma_f32_16x16x32_f16") == 128 and body.count("ds_read_b128") == 32
    assert body.count("global_load_lds_dwordx4") == 16 and body.count("s_barrier") == 1 and body.count("asm volatile(") == 1
    # nothing of K-tile g is read behind the barrier, nothing of K-tile g + 1 in front of it
    front, behind = body.split("s_barrier")
    assert front.count("ds_read_b128") == 22 and behind.count("ds_read_b128") == 10
    assert front.index("%[san]") > front.rindex("%[ra0] offset") and "%[san]" not in behind       # the next K-tile's address replaces ra0 behind its last use


def test_tile16_gemm_stream_waits_for_every_fragment_it_uses():
    """An independent reading of the generated 16x16x32 K-tile streams (all variants in gemm_ktile16_mfma.inc): replay the instruction
    text with the LDS return queue (reads return in order; `s_waitcnt lgkmcnt(n)` = at most n outstanding) and check that (i) no MFMA
    reads a fragment register whose ds_read may still be in flight, (ii) no ds_read overwrites a register while an OLDER read into the
    same register is still in flight, (iii) every accumulator is used exactly once per 32-deep slab, by the W tile / X tile pair its name
    says, (iv) the barrier is preceded by lgkmcnt(0) and vmcnt(8), and nothing of the next K-tile's stage (addresses made from san / sbn)
    is read in front of it."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "bonito_amd", "csrc", "gemm_ktile16_mfma.inc")).read()
    bodies = re.findall(r"asm volatile\(\"(.*?)\"\n\s*: ", text, flags=re.S)
    assert len(bodies) == 8                      # plain, first, and the three parked-store flavours of each
    for body in bodies:
        ins = [ln.strip().strip('"').replace("\\n\\t", "").strip() for ln in body.splitlines()]
        ins = [i for i in ins if i]
        fifo, used, next_stage_addr = [], {}, set()
        seen_barrier = False
        for k, i in enumerate(ins):
            m = re.match(r"v_mfma_f32_16x16x32_f16 %\[(c\d_\d)\], %\[(fb(\d)_(\d))\], %\[(fa(\d))\], (?:%\[(c\d_\d)\]|0)$", i)
            if m:
                c, fb, slab, j, fa, ti = m.group(1), m.group(2), int(m.group(3)), int(m.group(4)), m.group(5), int(m.group(6))
                assert fb not in fifo and fa not in fifo, (k, i, fifo)
                assert c == "c%d_%d" % (ti, j) and (m.group(7) in (None, c))
                used.setdefault(c, []).append(slab)
                continue
            m = re.match(r"ds_read_b128 %\[(\w+)\], %\[(\w+)\] offset:\d+$", i)
            if m:
                assert m.group(1) not in fifo, (k, i)
                if m.group(2) in next_stage_addr:
                    assert seen_barrier, (k, i)
                fifo.append(m.group(1))
                continue
            m = re.match(r"s_waitcnt lgkmcnt\((\d+)\)$", i)
            if m:
                del fifo[:max(0, len(fifo) - int(m.group(1)))]
                continue
            m = re.match(r"v_add_u32_e32 %\[(\w+)\], %\[(san|sbn)\], ", i)
            if m:
                next_stage_addr.add(m.group(1))
                continue
            m = re.match(r"v_add_u32_e32 %\[(\w+)\], %\[(sa|sb)\], ", i)
            if m:
                next_stage_addr.discard(m.group(1))
                continue
            if i == "s_barrier":
                assert not fifo and ins[k - 1] == "s_waitcnt vmcnt(8)" and ins[k - 2] == "s_waitcnt lgkmcnt(0)"
                seen_barrier = True
        assert seen_barrier and not fifo                              # the stream ends with lgkmcnt(0)
        assert len(used) == 64 and all(v == [0, 1] for v in used.values())


@pytest.mark.parametrize("preset,name", [("plain", "ringstep3_mfma.inc"), ("paired", "ringstep3p_mfma.inc"), ("unrolled", "ringstep3u_mfma.inc"),
                                         ("rec", "ringstep3r_mfma.inc")])
def test_ring_step_streams_match_their_generator(tmp_path, preset, name):
    """bonito_amd/csrc/ringstep3_mfma.inc / ringstep3p_mfma.inc (the hand-scheduled instruction stream of a ring step of the paired
    recurrent kernel; the second one carries the section's DMA and validation too) are generated by tools/gen_ringstep.py
    --preset plain|paired: the committed files must be what the committed generator writes, and each must be ONE asm statement
    (the compiler can place nothing inside; tools/audit_ringstep.py is the guard for multi-statement streams)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_ringstep", os.path.join(root, "tools", "gen_ringstep.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    out = str(tmp_path / name)
    gen.main(["--preset", preset, "--out", out])
    committed = open(os.path.join(root, "bonito_amd", "csrc", name)).read()
    assert open(out).read() == committed
    assert committed.count("asm volatile(") == 1 and committed.count("v_mfma_f32_16x16x32_f16") == (36 if preset == "rec" else 72)
    # hazards the generator is responsible for: no transcendental result consumed by the next instruction
    lines = [ln.strip().strip('"').replace("\\n\\t", "") for ln in committed.splitlines() if ln.strip().startswith('"') or "asm volatile" in ln]
    for a, b in zip(lines, lines[1:]):
        if a.startswith(("v_exp_f32", "v_rcp_f32")) or "asm volatile(\"v_exp" in a:
            dst = a.split()[1].rstrip(",")
            assert dst not in b.split("//")[0].replace(",", " ").split()[2:], (a, b)


def test_unrolled_ring_step_stream_computes_what_the_paired_one_computes():
    """ringstep3u_mfma.inc (main loop of the paired kernel, unrolled over four steps) is scheduled differently from ringstep3p_mfma.inc
    (publish woven into the last MFMAs, plain stores, polls later, tile offsets as template constants) but must compute the same
    bits: every accumulator sees the same MFMAs in the same order, every cell the same gate arithmetic in the same order."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def body(name):
        text = open(os.path.join(root, "bonito_amd", "csrc", name)).read()
        text = text[text.index("asm volatile(") + len("asm volatile("):text.index("\n        : ")]
        return [ln.strip().strip('"').replace("\\n\\t", "") for ln in text.splitlines()]

    paired, unrolled = body("ringstep3p_mfma.inc"), body("ringstep3u_mfma.inc")
    for acc in ["v[232:235]", "v[236:239]", "v[240:243]", "%[xa0]", "%[xa1]", "%[xa2]"]:
        seq = [[ln for ln in b if ln.startswith("v_mfma") and ln.split()[1] == acc + ","] for b in (paired, unrolled)]
        assert len(seq[0]) == 12 and seq[0] == seq[1], acc
    for m in range(3):
        regs = re.compile(r"\bv(%s)\b|%%\[[ec]%d\]" % ("|".join(str(232 + 4 * m + i) for i in range(4)), m))
        seq = [[ln for ln in b if not ln.startswith(("v_mfma", "v_cvt_f16")) and regs.search(ln)] for b in (paired, unrolled)]
        assert len(seq[0]) == 35 and seq[0] == seq[1], m
    # the publish: the same three conversions, 2-byte writes and the 8-byte read; the stores plain in the unrolled stream
    for pat in ("v_cvt_f16_f32", "ds_write_b16", "ds_read_b64"):
        assert [ln for ln in paired if ln.startswith(pat)] == [ln for ln in unrolled if ln.startswith(pat)]
    assert sum(ln.startswith("global_store_dwordx2") for ln in unrolled) == 3 and not any("sc1" in ln for ln in unrolled if ln.startswith("global_store"))
    assert sum(ln.startswith("global_load_lds_dwordx4") for ln in unrolled) == 6
    # the validation's vmcnt leaves exactly the vector-memory operations issued behind the last poll outstanding (in-order counter), and the
    # read-back of the polled quarter comes behind it; the same rule in the generic stream
    for b in (paired, unrolled):
        polls = [i for i, ln in enumerate(b) if ln.startswith("global_load_lds_dwordx4") and "%[exo]" in ln]
        waits = [i for i, ln in enumerate(b) if ln.startswith("s_waitcnt vmcnt(")]
        assert len(polls) == 3 and len(waits) == 1 and waits[0] > polls[-1]
        younger = sum(ln.startswith(("global_load_lds", "global_store")) for ln in b[polls[-1] + 1:waits[0]])
        assert b[waits[0]] == "s_waitcnt vmcnt(%d)" % younger
        reads = [i for i, ln in enumerate(b) if ln.startswith("ds_read_b128 v[22")]
        assert len(reads) == 3 and min(reads) > waits[0]


def test_bs2_constants_header_matches_its_generator(tmp_path):
    """include/bh_bs2.h (polynomial coefficients of the deterministic exp / log shared by beam.hip and oracle/crf_oracle.c) is what
    tools/gen_bs2_coeffs.py writes; both sides include the SAME file, which is what makes the guide rows bit-identical."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "bh_bs2.h"
    subprocess.run([sys.executable, os.path.join(root, "tools", "gen_bs2_coeffs.py"), str(out)], check=True, capture_output=True)
    assert out.read_text() == open(os.path.join(root, "include", "bh_bs2.h")).read()
    for path in (os.path.join(root, "oracle", "crf_oracle.c"), os.path.join(root, "bonito_amd", "csrc", "beam.hip")):
        assert "bh_bs2.h" in open(path).read()


def test_profile_classes_of_the_binding_match_the_header():
    """bh_encoder_profile_read fills BH_PROF_CLASSES floats: the Python handle's class names (round 6: fc1 and the attention kernel have
    classes of their own) must be exactly the header's enumerators, in order."""
    import re
    from bonito_amd.engine import HipEncoder
    text = open(os.path.join(ROOT, "include", "bonito_hip.h")).read()
    enum = text[text.index("enum { BH_PROF_CONV"):]
    enum = enum[:enum.index("};")]
    enum = re.sub(r"/\*.*?\*/", "", enum, flags=re.S)
    names = re.findall(r"BH_PROF_(\w+)\s*=\s*(\d+)", enum)
    table = {name.lower(): int(v) for name, v in names}
    n = table.pop("classes")
    assert n == len(HipEncoder.PROF_CLASSES) == len(table)
    for i, cls in enumerate(HipEncoder.PROF_CLASSES):
        assert table[cls] == i, (cls, i, table)


def test_option_table_header_and_library_agree():
    """The process-wide knobs exist once, as the rows of csrc/options.cpp: every row is described (quoted) in the knob comment of
    include/bonito_hip.h, that comment quotes nothing that is not a row, and bh_set_option takes every row's name with its default
    and refuses a name that is no row."""
    rows = re.findall(r"^\s*\{BH_OPT\((\w+)\),\s*(-?\d+),\s*Norm::\w+,\s*\"[^\"]+\"\},?\s*$",
                      open(os.path.join(ROOT, "bonito_amd", "csrc", "options.cpp")).read(), flags=re.M)
    names = [n for n, _ in rows]
    assert len(names) >= 20 and len(set(names)) == len(names)
    header = open(os.path.join(ROOT, "include", "bonito_hip.h")).read()
    comment = header[header.index("/* Process-wide knobs"):header.index("int bh_set_option(")]
    quoted = set(re.findall(r"\"(\w+)\"", comment))
    assert set(names) - quoted == set(), "not described in the header's knob comment"
    assert quoted - set(names) == set(), "quoted in the header's knob comment, but no row of the option table"
    handle = _lib.lib()
    for name, default in rows:
        assert handle.bh_set_option(name.encode(), int(default)) == 0, name
    assert handle.bh_set_option(b"no_such_option", 0) != 0
    assert "unknown option 'no_such_option'" in _lib.last_error()


def test_lstm_family_enum_of_the_binding_matches_the_header():
    text = open(os.path.join(ROOT, "include", "bonito_hip.h")).read()
    enum = text[text.index("enum bh_lstm_family {"):]
    enum = re.sub(r"/\*.*?\*/", "", enum[:enum.index("};")], flags=re.S)
    table = {name.lower(): int(v) for name, v in re.findall(r"BH_LSTM_(\w+)\s*=\s*(\d+)", enum)}
    assert table == _lib.LSTM_FAMILIES and sorted(table.values()) == list(range(8))
    # the internal launchers use the same enumerators: there is no second definition
    assert "enum bh_lstm_family {" not in open(os.path.join(ROOT, "bonito_amd", "csrc", "kernels.h")).read()


def test_conv_kernel_codes_of_the_binding_match_the_header():
    text = open(os.path.join(ROOT, "include", "bonito_hip.h")).read()
    enum = text[text.index("enum bh_conv_kernel {"):]
    enum = re.sub(r"/\*.*?\*/", "", enum[:enum.index("};")], flags=re.S)
    table = {name.lower(): int(v) for name, v in re.findall(r"BH_CONV_K_(\w+)\s*=\s*(\d+)", enum)}
    assert table == _lib.CONV_KERNELS and len(set(table.values())) == len(table)
    assert "#define BH_CONV_K_IGEMM(ntt, fs) (BH_CONV_K_IGEMM_BASE + 10 * (ntt) + (fs))" in text
    assert _lib.conv_igemm_code(4, True) == 141 and _lib.conv_igemm_code(1, False) == 110


@pytest.mark.parametrize("kw", [dict(Cout3=128), dict(Cout3=0), dict(K2=7), dict(K2=0), dict(K1=9), dict(K1=0), dict(K3=21), dict(K3=18),
                                dict(s3=8), dict(s3=64)], ids=lambda kw: "%s_%d" % next(iter(kw.items())))
def test_conv_front3_refuses_a_shape_without_an_instance(kw):
    """bh_conv1d_front3 checks its shape predicate in front of any device call (the pointers below are never read): the 96-channel
    instance must not be handed any Cout3 != 384, nor packed weights of another K2 / K3 than its fragment loads assume."""
    import ctypes as C
    a = dict(K1=5, K2=5, K3=19, s3=6, Cout3=384)
    a.update(kw)
    p = C.c_void_p(4096)
    rc = _lib.lib().bh_conv1d_front3(p, 3, 1600, p, p, a["K1"], 2, 1, -0.5, 3.5, p, p, a["K2"], 2, 1, -0.5, 3.5, p, p, a["Cout3"], a["K3"], a["s3"],
                                     9, 1, -0.5, 3.5, p, 384, 3 * 384, None)
    assert rc != 0 and "no instance for K1=%d K2=%d Cout3=%d K3=%d stride3=%d" % (a["K1"], a["K2"], a["Cout3"], a["K3"], a["s3"]) in _lib.last_error()


def test_conv_front3_argument_checks():
    import ctypes as C
    p = C.c_void_p(4096)

    def call(sig=p, w1=p, w2=p, w3=p, out=p, N=3, L0=1600, s3=6):
        rc = _lib.lib().bh_conv1d_front3(sig, N, L0, w1, None, 5, 2, 1, -0.5, 3.5, w2, None, 5, 2, 1, -0.5, 3.5, w3, None, 384, 19, s3, 9, 1, -0.5, 3.5,
                                         out, 384, 3 * 384, None)
        return rc, _lib.last_error()
    for kw in (dict(sig=None), dict(w1=None), dict(w2=None), dict(w3=None), dict(out=None), dict(N=0), dict(s3=0), dict(s3=-1)):
        rc, msg = call(**kw)
        assert rc != 0 and "bad arguments" in msg, kw
    rc, msg = call(L0=0)
    assert rc != 0 and "too short" in msg


def _family_call(family, H, T=3, N=32, flags=0, x=4096, w=True, h_out=8192):
    import ctypes as C
    import numpy as np
    wt = np.zeros(4, np.float32)            # never read: every case below is refused by the argument checks in front of any device call
    wp = wt.ctypes.data_as(C.c_void_p) if w else None
    fam = _lib.LSTM_FAMILIES[family] if isinstance(family, str) else family
    rc = _lib.lib().bh_lstm_layer_family(C.c_void_p(x), wp, wp, None, T, N, H, 0, fam, flags, C.c_void_p(h_out), None)
    return rc, _lib.last_error()


@pytest.mark.parametrize("family,H", [("wave", 544), ("wave", 48), ("fused", 1024), ("stream", 96), ("stream", 1088), ("wgx", 320), ("wgx", 32),
                                      ("wgx2", 512), ("wgx2", 160), ("cta", 192), ("cta", 256), ("wide", 512), ("wide", 704), ("wide", 960),
                                      ("wide", 1152)])
def test_lstm_layer_family_refuses_a_width_without_an_instance(family, H):
    rc, msg = _family_call(family, H)
    assert rc != 0 and "has no instance for hidden size %d" % H in msg


def test_lstm_layer_family_argument_checks():
    for kw in (dict(x=0), dict(w=False), dict(h_out=0), dict(x=8192)):
        rc, msg = _family_call("fused", 96, **kw)
        assert rc != 0 and "null pointer, or x and h_out are one buffer" in msg, kw
    for kw in (dict(T=0), dict(N=0), dict(N=-16)):
        rc, msg = _family_call("fused", 96, **kw)
        assert rc != 0 and "must be positive" in msg, kw
    for fam in ("q8", -1, 8):
        rc, msg = _family_call(fam, 96)
        assert rc != 0 and "not an fp16 family" in msg, fam
    for fam, N in (("fused", 24), ("wgx", 40), ("cta", 8), ("wide", 16), ("wide", 48)):      # rings of 16 chunks, 32 for the wide kernel
        rc, msg = _family_call(fam, 1024 if fam == "wide" else 96, N=N)
        assert rc != 0 and "no multiple of the family's ring" in msg, (fam, N)
    for fam, flags in (("fused", 2), ("wgx", 3), ("wide", 4), ("cta", 8)):                    # bit 1 means something to the wide kernel only
        rc, msg = _family_call(fam, 1024 if fam == "wide" else 96, flags=flags)
        assert rc != 0 and "flags %d not understood" % flags in msg, (fam, flags)
    rc, msg = _family_call("fused", 96, x=4100)
    assert rc != 0 and "16-byte aligned" in msg
    # more rings than one launch holds (32 at H = 512 on 256 CUs; 16 x 4096 chunks are too many for any device)
    rc, msg = _family_call("wave", 512, N=16 * 4096)
    assert rc != 0 and "one launch of family 0 holds" in msg
