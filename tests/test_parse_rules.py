"""The libffm parsers against an independent reference, bit for bit.

Four parsers -- native.parse_libffm (csrc/io/reader.cpp), Engine.parse_text on
the CPU backend, Engine.parse_text on the GPU (csrc/hip/kernels_parse.hip) and,
where a case concerns it, TextStream through parse_text_file -- against
xflow_amd/testing/ffm_ref.py (pure Python, the C library's strtod, the Python
std_hash): exact equality of labels, row_ptr, fgid, keys, rows, features,
nnz_per_row and nnz_used.  No tolerances.

Engine.parse_text is called directly so the test owns the buffers: the text
sits in a tensor of n + 64 bytes whose tail is a poison that would parse as
data (and, in a second run, zeros), and the outputs are exact-length views
into sentinel-filled tensors whose guards are checked after every parse.

* a hand-written case table (feature text lengths around the 8 / 16 byte
  edges of the in-register hash, line alignment, block lengths around the
  16-byte and 4 KB chunk edges, line shapes, labels around the 1e-7
  threshold, field ids through the integer path and through atof, row_mod);
* a seeded grammar fuzz whose corpus coverage is asserted from the
  reference's own outputs;
* one block of 4.2 M short lines that takes every multi-level scan and
  grid-stride loop of the device parser past its first iteration;
* the capacity and error contracts.
"""
import functools
import random
from fractions import Fraction

import numpy as np
import pytest
import torch

from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig
from xflow_amd.data.textstream import parse_text_file
from xflow_amd.engine import Engine
from xflow_amd.testing import ffm_ref

GUARD = 16
FILL = {"keys": (torch.int64, 0x5A5A5A5A5A5A5A5A), "fgid": (torch.int32, 0x5A5A5A5A),
        "row_ptr": (torch.int32, 0x5A5A5A5A), "labels": (torch.float32, 7.5)}
POISON = (b"\n1\t9:zz:1\n:" * 6)[:64]
ZEROS = bytes(64)
ARRAYS = ("labels", "row_ptr", "fgid", "keys")


# ---------------------------------------------------------------- harness

def _engine(device):
    return Engine(ModelConfig(kind="lr"), OptimConfig(), EngineConfig(table_log2_cap=12),
                  device=device)


@pytest.fixture(scope="module")
def cpu_engine():
    return _engine(torch.device("cpu"))


@pytest.fixture(scope="module")
def gpu_engine(gpu_device):
    return _engine(gpu_device)


def _text_tensor(block: bytes, pad: bytes, device, extra: int = 64):
    n = len(block)
    t = torch.frombuffer(bytearray(block + pad[:extra]), dtype=torch.uint8)
    assert t.numel() == n + extra
    return t.to(device)


def _outputs(rows: int, nnz: int, device):
    """Exact-length views into sentinel-filled tensors: name -> (whole, view)."""
    sizes = {"keys": nnz, "fgid": nnz, "row_ptr": rows + 1, "labels": rows}
    bufs = {}
    for name, size in sizes.items():
        dt, fill = FILL[name]
        whole = torch.full((GUARD + size + GUARD,), fill, dtype=dt, device=device)
        bufs[name] = (whole, whole[GUARD:GUARD + size])
    return bufs


def _assert_guards(bufs, untouched: bool = False):
    for name, (whole, view) in bufs.items():
        w = whole.cpu()
        fill = torch.tensor(FILL[name][1], dtype=w.dtype)
        assert bool((w[:GUARD] == fill).all()), "%s: written before the array" % name
        assert bool((w[GUARD + view.numel():] == fill).all()), "%s: written past the array" % name
        if untouched:
            body = w[GUARD:GUARD + view.numel()]
            if name == "row_ptr":  # (row_ptr[0] = 0 is written before the counts are known)
                body = body[1:]
            assert bool((body == fill).all()), "%s: written by a parse that failed" % name


def _parse(eng, block: bytes, rows_cap: int, nnz_cap: int, row_mod: int = 1, pad: bytes = POISON):
    """Engine.parse_text on owned buffers -> host dict (guards checked)."""
    dev = eng.device
    text = _text_tensor(block, pad, dev)
    bufs = _outputs(rows_cap, nnz_cap, dev)
    out = {k: v[1] for k, v in bufs.items()}
    try:
        rows, nnz, lmin, lmax, nused = eng.parse_text(text, len(block), out, row_mod)
    except RuntimeError:
        _assert_guards(bufs, untouched=True)
        raise
    _assert_guards(bufs)
    assert rows <= rows_cap and nnz <= nnz_cap
    return {"labels": out["labels"][:rows].cpu().numpy(),
            "row_ptr": out["row_ptr"][:rows + 1].cpu().numpy(),
            "fgid": out["fgid"][:nnz].cpu().numpy(), "keys": out["keys"][:nnz].cpu().numpy(),
            "rows": rows, "features": nnz, "nnz_per_row": lmin if lmin == lmax else 0,
            "nnz_used": nused}


def _check(got: dict, ref: dict, what: str = ""):
    assert got["rows"] == ref["rows"], what
    assert got["features"] == ref["features"], what
    for k in ARRAYS:
        g = np.asarray(got[k])
        if k == "keys":
            g = g.view(np.uint64)
        assert g.dtype == ref[k].dtype, (what, k)
        np.testing.assert_array_equal(g, ref[k], err_msg="%s %s" % (what, k))
    assert got["nnz_per_row"] == ref["nnz_per_row"], what
    assert got["nnz_used"] == ref["nnz_used"], what


def _check_engine(eng, block: bytes, ref: dict, row_mod: int = 1, what: str = ""):
    """Exact-size arrays, poison and then zero padding after the block."""
    for pad in (POISON, ZEROS):
        got = _parse(eng, block, ref["rows"], ref["features"], row_mod, pad)
        _check(got, ref, "%s pad=%s" % (what, "poison" if pad is POISON else "zero"))


def _check_native(native, block: bytes, ref: dict, row_mod: int = 1, what: str = ""):
    b = native.parse_libffm(block)
    got = {k: np.asarray(b[k]) for k in ARRAYS}
    lens = np.diff(got["row_ptr"])
    rows = len(got["labels"])
    got.update(rows=rows, features=len(got["keys"]),
               nnz_per_row=int(lens[0]) if rows and (lens == lens[0]).all() else 0,
               nnz_used=int(got["row_ptr"][rows - rows % row_mod]))
    _check(got, ref, what)


def _check_stream(eng, tmp_path, block: bytes, ref: dict, what: str = ""):
    """The block as a one-block file through TextStream."""
    p = tmp_path / "block-00000"
    p.write_bytes(block)
    got = parse_text_file(eng, str(p), len(block) + 16)
    if ref["rows"] == 0:
        assert got == []
        return
    assert len(got) == 1
    g = dict(got[0])
    g["features"] = len(g["keys"])
    _check(g, ref, what)


# ------------------------------------------------------------- case table

ALNUM = b"0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJ"
ROW = b"1\t7:abcdefgh:1 8:xy\n"


def _threshold_labels():
    """25-digit mantissas just above and just below the point where strtod
    starts to return the double above 1e-7 (the threshold's own double)."""
    t = Fraction(ffm_ref.THRESHOLD)
    mid = t + Fraction(1, 2 ** 77)  # half an ulp (2^-76) above: the rounding boundary
    lo = int(mid * 10 ** 31)        # 25 digits; mid is no 25-digit decimal
    assert len(str(lo)) == 25 and Fraction(lo, 10 ** 31) < mid < Fraction(lo + 1, 10 ** 31)
    return b"%de-31" % (lo + 1), b"%de-31" % lo


def _fill_to(n: int, final_newline: bool) -> bytes:
    row = b"1\t2:ab:1 3:c\n"
    t = (row * (n // len(row) + 1))[:n]
    return t[:-1] + b"\n" if final_newline and n else t


def _build_cases():
    c = {}

    def add(cid, block, row_mod=1):
        assert cid not in c, cid
        c[cid] = (bytes(block), row_mod)

    # feature text length
    for L in range(41):
        f = ALNUM[:L]
        add("flen-3part-%d" % L, b"1\t3:" + f + b":1 4:x:1\n")
        add("flen-2part-lf-%d" % L, b"0\t3:" + f + b"\n")
        add("flen-2part-crlf-%d" % L, b"1\t3:" + f + b"\r\n")
        add("flen-2part-crcrlf-%d" % L, b"1\t3:" + f + b"\r\r\n")
    add("flen-cr-mid-3part", b"1\t3:ab\rcd:1\n")
    add("flen-cr-mid-2part", b"1\t3:ab\rcd\r\n")
    add("flen-cr-end-3part-kept", b"1\t3:ab\r:1\n")
    add("flen-cr-2part-before-space", b"1\t3:ab\r 4:cd\r\r 5:e\n")
    add("flen-only-cr", b"1\t3:\r\r\r\n")
    add("flen-20-cr-strip-to-0", b"1\t3:" + b"\r" * 20 + b"\n")
    add("flen-20-strip-to-10", b"1\t3:abcdefghij" + b"\r" * 10 + b"\n")
    add("flen-20-strip-to-16", b"1\t3:abcdefghijklmnop" + b"\r" * 4 + b"\n")
    add("flen-16-cr", b"1\t3:" + ALNUM[:16] + b"\r\n")
    add("flen-17-cr", b"1\t3:" + ALNUM[:17] + b"\r\n")
    for L in (1, 3, 7, 8, 9, 12, 15, 16, 17, 20):
        hi = bytes(0x80 + (i * 37 + L) % 0x80 for i in range(L))
        add("bytes-high-%d" % L, b"1\t3:" + hi + b":1 4:" + hi + b"\n")
        add("bytes-ff-%d" % L, b"1\t3:" + b"\xff" * L + b":1\n")
        add("bytes-nul-%d" % L, b"1\t3:" + b"\x00" * L + b":1 4:" + b"a\x00" * L + b"\n")

    # alignment
    for off in range(16):
        pre = b"" if off == 0 else b"x" * (off - 1) + b"\n"
        add("align-line-start-%d" % off, pre + ROW + ROW)
    add("align-feature-straddles-16", b"x" * 7 + b"\n" + b"1\t3:0123456789:1\n")
    add("align-feature-straddles-4096", b"x" * 4085 + b"\n" + b"1\t3:0123456789ab:1\n")
    add("align-long-feature-straddles-4096", b"x" * 4075 + b"\n" + b"1\t3:" + ALNUM[:30] + b"\n")
    add("align-id-straddles-4096", b"x" * 4091 + b"\n" + b"1\t1234567:a 1.5e1:b\n")
    add("align-label-straddles-4096", b"x" * 4089 + b"\n" + b"0.00000011\t1:a\n")

    # block length
    add("len-0", b"")
    add("len-1-newline", b"\n")
    add("len-1-tab", b"\t")
    add("len-1-digit", b"1")
    add("len-2-tab-newline", b"\t\n")
    add("len-2-label-tab", b"1\t")
    add("len-2-newlines", b"\n\n")
    add("len-3-newlines", b"\n\n\n")
    add("len-4-newlines", b"\n\n\n\n")
    for n in (15, 16, 17, 4095, 4096, 4097, 8192):
        add("len-%d-cut" % n, _fill_to(n, False))
        add("len-%d-newline-last" % n, _fill_to(n, True))
    add("len-newline-at-15-and-16", b"1\t2:" + b"a" * 11 + b"\n\n" + ROW)
    t = _fill_to(4095 - 20, True)
    add("len-newline-at-4095-and-4096", t + b"x" * 20 + b"\n\n" + ROW)
    assert c["len-newline-at-4095-and-4096"][0][4095:4097] == b"\n\n"
    add("len-16-no-final-newline", b"1\t2:abcdefghijkl")
    add("len-4096-no-final-newline", _fill_to(4096 - 16, True) + b"1\t2:abcdefghijkl")
    add("len-no-newline-row", b"1\t2:a:1 3:b")
    add("len-no-newline-no-row", b"abc")

    # line shapes
    add("line-no-tab", b"no tab here\n" + ROW)
    add("line-only-tab", b"\t\n" + ROW)
    add("line-tab-last-byte", ROW + b"1\t")
    add("line-tab-before-newline", b"0.5\t\n")
    add("line-second-tab", b"1\t1:a:1 \t2:b:1 3\t4:c:1 5:d\te:1\n")
    add("line-double-trailing-spaces", b"1\t  1:a:1  2:b:1   \n")
    add("line-odd-tokens", b"1\t: :: a: :a 5: :z:1\n")
    add("line-no-colon-between", b"1\t1:a:1 nocolon 2:b:1\n")
    add("line-no-colon-only", b"1\tabc def 7\n0\t1:a\n")
    add("line-lone-crlf", b"\r\n" + ROW + b"\r\n")
    add("line-space-before-tab", b"1 \t1:a:1\n 1\t2:b:1\n")

    # labels
    above, below = _threshold_labels()
    labels = [b"0.0000001", b"1e-7", b"1.0000000000000002e-7", b"0.00000010000001",
              b"1000000000000000000000000e-31", b"0.00000000000000000000001e16", above, below,
              b"1e-400", b"1e400", b"-0", b".5", b"5.", b"+.5e+1", b"1e", b"1e+", b"e5", b".",
              b"-", b"", b"inf", b"-inf", b"Infinity", b"nan", b"NAN", b"\v1", b"\f1", b"\r1",
              b"1,5", b"1 2", b"1\x002", b"\x001", b"0" * 62 + b"1", b"0" * 62 + b"10",
              b"0" * 63 + b"1", b"." + b"0" * 61 + b"9", b"0.00000009999999999999999",
              b"0.000000100000000000000001", b"-1e-7", b"1E-6", b"1e-6x"]
    for i, lab in enumerate(labels):
        add("label-%02d-%s" % (i, lab[:24].decode("latin-1").encode("unicode_escape").decode()),
            lab + b"\t1:a:1\n")

    # field ids
    ids = [b"007", b"+5", b"-0", b"2147483647", b"-2147483648", b"", b"-2147483647",
           b"1.9", b"-1.9", b"1e3", b"1e", b"12abc", b"abc", b"-", b"+-1", b"5\v", b"\v5",
           b"0.99999999999999999999", b"0." + b"9" * 68, b"0." + b"0" * 67 + b"9",
           b"2147483647.9", b"-2147483648.0", b"21474836.47e2", b"5\x006", b"+", b"-5",
           b"0000000000000000000012", b"1.0000000000000000000000001e9"]
    for i, fid in enumerate(ids):
        add("id-%02d-%s" % (i, fid[:24].decode("latin-1").encode("unicode_escape").decode()),
            b"1\t" + fid + b":a:1 9:z:1\n")

    # row_mod
    for rm in (1, 3, 8):
        for rows in (0, 2, 8, 9):
            fixed = b"".join(b"%d\t1:a%d:1 2:b:1 3:c\n" % (r & 1, r) for r in range(rows))
            ragged = b"".join(b"%d\t" % (r & 1) + b" ".join(b"%d:f%d:1" % (j, r) for j in range(r % 4))
                              + b"\n" for r in range(rows))
            add("rowmod-%d-rows-%d-fixed" % (rm, rows), fixed or b"no rows\n", rm)
            add("rowmod-%d-rows-%d-ragged" % (rm, rows), ragged or b"x\ny\n", rm)
    return c


CASES = _build_cases()
CASE_IDS = list(CASES)


@functools.lru_cache(maxsize=None)
def _case_ref(cid):
    block, row_mod = CASES[cid]
    return ffm_ref.parse(block, row_mod)


def test_case_table_premises():
    """What the table relies on, from the reference alone."""
    r = _case_ref
    above, below = _threshold_labels()
    assert ffm_ref.label_of(above) == 1.0 and ffm_ref.label_of(below) == 0.0
    assert ffm_ref.c_atof(b"1000000000000000000000000e-31") == ffm_ref.THRESHOLD
    assert r("flen-2part-crcrlf-15")["keys"][0] == r("flen-2part-lf-15")["keys"][0]
    assert r("flen-cr-end-3part-kept")["keys"][0] != r("flen-3part-2")["keys"][0]
    assert r("rowmod-8-rows-2-fixed")["nnz_used"] == 0
    assert r("rowmod-3-rows-8-fixed")["nnz_per_row"] == 3
    assert r("rowmod-3-rows-8-ragged")["nnz_per_row"] == 0
    assert r("len-0")["rows"] == 0 and r("len-1-tab")["rows"] == 1
    with pytest.raises(ffm_ref.Unsupported):
        ffm_ref.parse(b"1\t0x1p3:a:1\n")
    with pytest.raises(ffm_ref.Unsupported):
        ffm_ref.parse(b"0X.8\t1:a:1\n")
    with pytest.raises(ffm_ref.Unsupported):
        ffm_ref.parse(b"1\t2147483648:a:1\n")
    with pytest.raises(ffm_ref.Unsupported):
        ffm_ref.parse(b"1\tnan:a:1\n")


@pytest.mark.parametrize("cid", CASE_IDS)
def test_case_native(native, cid):
    block, row_mod = CASES[cid]
    _check_native(native, block, _case_ref(cid), row_mod, cid)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_case_cpu(cpu_engine, cid):
    block, row_mod = CASES[cid]
    _check_engine(cpu_engine, block, _case_ref(cid), row_mod, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", CASE_IDS)
def test_case_gpu(gpu_engine, cid):
    block, row_mod = CASES[cid]
    _check_engine(gpu_engine, block, _case_ref(cid), row_mod, cid)


STREAM_CASES = ["flen-2part-crcrlf-16", "len-1-tab", "len-4096-no-final-newline",
                "line-odd-tokens", "len-no-newline-no-row",
                next(c for c in CASE_IDS if c.startswith("label-04-"))]


@pytest.mark.parametrize("cid", STREAM_CASES)
def test_case_stream_cpu(cpu_engine, tmp_path, cid):
    _check_stream(cpu_engine, tmp_path, CASES[cid][0], ffm_ref.parse(CASES[cid][0]), cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", STREAM_CASES)
def test_case_stream_gpu(gpu_engine, tmp_path, cid):
    _check_stream(gpu_engine, tmp_path, CASES[cid][0], ffm_ref.parse(CASES[cid][0]), cid)


# ------------------------------------------------------------ grammar fuzz

FUZZ_BLOCKS = 200
_FEAT_BYTES = bytes(b for b in range(256) if b not in b"\n\t :")
_FUZZ_LABELS = [b"0", b"1", b"0", b"1", b"-1", b"0.5", b"", b"1e-7", b"0.0000001", b"1.0000000000000002e-7",
                b"1000000000000000000000000e-31", b"0.00000000000000000000001e16", b"1e-400",
                b"1e400", b"-0", b".5", b"5.", b"+.5e+1", b"1e", b"e5", b".", b"-", b"inf", b"-inf",
                b"nan", b"\v1", b"1,5", b"1 2", b"1\x002", b"0" * 62 + b"1", b"0" * 63 + b"1",
                b"  1.0e0", b"\r0.3"]
_FUZZ_IDS = [b"0", b"1", b"7", b"38", b"007", b"+5", b"-0", b"-3", b"2147483647", b"-2147483648", b"",
             b"1.9", b"-1.9", b"1e3", b"1e", b"12abc", b"abc", b"-", b"+-1", b"5\v", b"\v5",
             b"0.99999999999999999999", b"0." + b"9" * 68, b"\t4", b"5\x006"]
_FUZZ_ODD = [b":", b"::", b"a:", b":a", b"5:", b":z:1", b"nocolon", b"x", b"123", b"\r", b"", b""]
_FUZZ_FLENS = [0, 1, 3, 7, 8, 9, 15, 16, 17, 18, 24, 33, 40]


def _fuzz_number(rng, pool, of):
    if rng.random() < 0.25:
        digits = "".join(rng.choice("0123456789") for _ in range(rng.randint(1, 26)))
        k = rng.randint(0, len(digits))
        s = (digits[:k] + "." + digits[k:]) if rng.random() < 0.6 else digits
        if of is ffm_ref.label_of:  # around the threshold / any exponent
            s += "e%d" % (-7 - k + rng.randint(-1, 1) if rng.random() < 0.7 else rng.randint(-30, 30))
            s = rng.choice(["", "", "-", "+"]) + s
        else:  # a field id stays an int32: at most 9 digits before the point
            s = rng.choice(["", "", "-", "+"]) + s[:9 + (1 if "." in s[:9] else 0)]
        b = s.encode()
    else:
        b = rng.choice(pool)
    of(b)  # (raises Unsupported for a construct the reference excludes)
    return b


def _fuzz_feature(rng):
    L = rng.choice(_FUZZ_FLENS) if rng.random() < 0.8 else rng.randint(0, 40)
    src = ALNUM if rng.random() < 0.7 else _FEAT_BYTES
    return bytes(rng.choice(src) for _ in range(L))


def _fuzz_block(seed: int) -> bytes:
    rng = random.Random(seed)
    target = rng.randint(1024, 7800)
    out = bytearray()
    lines = 0
    while len(out) < target:
        u = rng.random()
        if u < 0.10:
            line = rng.choice([b"x", b"no tab here", b"1 2:3:4", b":", b"0.5 7:a:1"])
        elif u < 0.16 and len(out) >= 2 * (lines + 2):
            line = b""  # (an empty line only where the n/2 + 2 line bound has room)
        else:
            toks = []
            for _ in range(rng.choice([0, 0, 1, 2, 3, 5, 8, 20])):
                v = rng.random()
                if v < 0.25:
                    toks.append(rng.choice(_FUZZ_ODD))
                    continue
                fid = _fuzz_number(rng, _FUZZ_IDS, ffm_ref.field_id_of)
                if v < 0.30:
                    fid = b"\t" + fid
                    ffm_ref.field_id_of(fid)
                tok = fid + b":" + _fuzz_feature(rng)
                if v < 0.55:
                    tok += rng.choice([b"", b"", b"\r", b"\r\r"])  # 2-part
                else:
                    tok += b":" + rng.choice([b"1", b"0.5", b"", b"1:2"])
                toks.append(tok)
            line = _fuzz_number(rng, _FUZZ_LABELS, ffm_ref.label_of) + b"\t" + b" ".join(toks)
        out += line + rng.choice([b"\n", b"\n", b"\n", b"\r\n", b"\r\r\n"])
        lines += 1
    if seed % 4 == 0:
        out = out[:-1]  # no final newline
    block = bytes(out)
    assert block.count(b"\n") + 1 <= len(block) // 2 + 2
    return block


@functools.lru_cache(maxsize=None)
def _corpus():
    """[(block, reference parse)], its coverage asserted from the reference's
    outputs before any parser under test sees a block.  The generator checks
    every number it emits against the reference's exclusions, so no block is
    discarded."""
    blocks = [_fuzz_block(1000 + i) for i in range(FUZZ_BLOCKS)]
    corpus = [(b, ffm_ref.parse(b, 1 + i % 3)) for i, b in enumerate(blocks)]
    assert all(1024 <= len(b) <= 8192 for b in blocks)
    st = [r["stats"] for _, r in corpus]
    flens = set().union(*(s["flens"] for s in st))
    assert sum(s["no_row_lines"] for s in st) > 0
    assert sum(s["featureless_rows"] for s in st) > 0
    assert sum(s["no_colon_tokens"] for s in st) > 0
    assert sum(s["empty_tokens"] for s in st) > 0
    assert sum(s["cr_stripped"] for s in st) > 0
    assert {0, 7, 8, 9, 15, 16, 17} <= flens and max(flens) > 17
    assert sum(s["ids_atof"] for s in st) > 0
    assert sum(s["labels_pos"] for s in st) > 0 and sum(s["labels_neg"] for s in st) > 0
    assert any(s["no_final_newline"] for s in st) and not all(s["no_final_newline"] for s in st)
    return corpus


def test_fuzz_corpus_coverage():
    assert len(_corpus()) == FUZZ_BLOCKS


def test_fuzz_native(native):
    for i, (block, ref) in enumerate(_corpus()):
        _check_native(native, block, ref, 1 + i % 3, "fuzz block %d" % i)


def test_fuzz_cpu(cpu_engine):
    for i, (block, ref) in enumerate(_corpus()):
        _check_engine(cpu_engine, block, ref, 1 + i % 3, "fuzz block %d" % i)


@pytest.mark.gpu
def test_fuzz_gpu(gpu_engine):
    for i, (block, ref) in enumerate(_corpus()):
        _check_engine(gpu_engine, block, ref, 1 + i % 3, "fuzz block %d" % i)


# ------------------------------------------------------------- large block

UNIT = b"1\t:\nx\n0\t\n\t:\n1\t1:a\nab\n"  # 21 bytes: 6 lines of 2..6 bytes, 4 rows, 3 features
REPS = 700_000
# a repetition past the first iteration of each loop, by the lines / bytes before it
LEVELS = (("k_scan_top carry (256 * 1024 lines)", 50_000),
          ("k_nl_scan carry (1024 chunks of 4 KB)", 250_000),
          ("k_line_count / k_line_emit grid stride (8192 * 256 lines)", 400_000),
          ("k_scan_reduce / k_scan_apply grid stride (4096 * 1024 lines)", 699_500))
LARGE_ROW_MOD = 3


@functools.lru_cache(maxsize=None)
def _large():
    u = ffm_ref.parse(UNIT)
    lines, rows, feats = u["stats"]["lines"], u["rows"], u["features"]
    assert len(UNIT) % 2 == 1 and (lines, rows, feats) == (6, 4, 3)
    n = len(UNIT) * REPS
    assert lines * REPS > 4096 * 1024 and n // 2 + 2 > lines * REPS
    assert LEVELS[0][1] * lines > 256 * 1024 and LEVELS[1][1] * len(UNIT) > 1024 * 4096
    assert LEVELS[2][1] * lines > 8192 * 256 and LEVELS[3][1] * lines > 4096 * 1024
    row_ptr = np.concatenate([[0], (np.arange(REPS, dtype=np.int64)[:, None] * feats
                                    + u["row_ptr"][None, 1:]).ravel()]).astype(np.int32)
    R = rows * REPS
    ref = {"labels": np.tile(u["labels"], REPS), "row_ptr": row_ptr,
           "fgid": np.tile(u["fgid"], REPS), "keys": np.tile(u["keys"], REPS),
           "rows": R, "features": feats * REPS, "nnz_per_row": 0,
           "nnz_used": int(row_ptr[R - R % LARGE_ROW_MOD])}
    return UNIT * REPS, ref, u


def _check_large(eng):
    block, ref, u = _large()
    rows, feats = u["rows"], u["features"]
    for pad in (POISON, ZEROS):
        got = _parse(eng, block, ref["rows"], ref["features"], LARGE_ROW_MOD, pad)
        assert got["rows"] == ref["rows"] and got["features"] == ref["features"]
        for level, rep in LEVELS:
            np.testing.assert_array_equal(got["row_ptr"][rows * rep:rows * rep + rows + 1],
                                          feats * rep + u["row_ptr"], err_msg=level)
        _check(got, ref, "large block")


def test_large_block_cpu(cpu_engine):
    _check_large(cpu_engine)


@pytest.mark.gpu
def test_large_block_gpu(gpu_engine):
    _check_large(gpu_engine)


# ------------------------------------------- capacity and error contracts

GOOD = b"1\t1:a:1 2:bb:1\n0\t3:c\r\n"
EMPTY_LINES = b"\n" * 50 + b"1\t1:a:1\n"


def _check_capacity(eng):
    ref = ffm_ref.parse(GOOD)
    _check(_parse(eng, GOOD, ref["rows"], ref["features"]), ref, "exact-size arrays")
    for dr, dn in ((1, 0), (0, 1)):
        with pytest.raises(RuntimeError, match="more rows / features"):
            _parse(eng, GOOD, ref["rows"] - dr, ref["features"] - dn)  # (sentinels: _parse)
        _check(_parse(eng, GOOD, ref["rows"], ref["features"]), ref, "after a short array")


def _check_empty_lines(eng):
    assert EMPTY_LINES.count(b"\n") > len(EMPTY_LINES) // 2 + 2
    ref = ffm_ref.parse(EMPTY_LINES)
    with pytest.raises(RuntimeError, match="more lines than n/2 \\+ 2"):
        _parse(eng, EMPTY_LINES, ref["rows"], ref["features"])
    good = ffm_ref.parse(GOOD)
    _check(_parse(eng, GOOD, good["rows"], good["features"]), good, "after the rejected block")


def test_capacity_cpu(cpu_engine):
    _check_capacity(cpu_engine)


@pytest.mark.gpu
def test_capacity_gpu(gpu_engine):
    _check_capacity(gpu_engine)


def test_mostly_empty_lines_rejected_cpu(cpu_engine):
    _check_empty_lines(cpu_engine)


@pytest.mark.gpu
def test_mostly_empty_lines_rejected_gpu(gpu_engine):
    _check_empty_lines(gpu_engine)


@pytest.mark.gpu
def test_misaligned_text_raises_gpu(gpu_engine):
    text = _text_tensor(b"x" + GOOD, POISON, gpu_engine.device)
    bufs = _outputs(2, 3, gpu_engine.device)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        gpu_engine.parse_text(text[1:], len(GOOD), {k: v[1] for k, v in bufs.items()})
    for name, (whole, _) in bufs.items():
        assert bool((whole == FILL[name][1]).all()), name


@pytest.mark.gpu
def test_short_text_tensor_raises_gpu(gpu_engine):
    text = _text_tensor(GOOD, POISON, gpu_engine.device, extra=31)
    bufs = _outputs(2, 3, gpu_engine.device)
    with pytest.raises(ValueError, match="n \\+ 32"):
        gpu_engine.parse_text(text, len(GOOD), {k: v[1] for k, v in bufs.items()})
    good = ffm_ref.parse(GOOD)
    _check(_parse(gpu_engine, GOOD, good["rows"], good["features"]), good, "after the short tensor")


DENSE = {"dense-colon-200": b"1\t" + b": " * 200 + b"\n",
         "dense-a-colon-200": b"1\t" + b"a: " * 200 + b"\n",
         "dense-colon-3000-rows": (b"1\t" + b": " * 30 + b"\n") * 100}


@pytest.mark.parametrize("cid", list(DENSE))
def test_dense_tokens_cpu(native, cpu_engine, tmp_path, cid):
    ref = ffm_ref.parse(DENSE[cid])
    assert ref["features"] > len(DENSE[cid]) // 4 + 2  # (more than the steady-state arrays hold)
    _check_native(native, DENSE[cid], ref, 1, cid)
    _check_engine(cpu_engine, DENSE[cid], ref, 1, cid)
    _check_stream(cpu_engine, tmp_path, DENSE[cid], ref, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(DENSE))
def test_dense_tokens_gpu(gpu_engine, tmp_path, cid):
    ref = ffm_ref.parse(DENSE[cid])
    _check_engine(gpu_engine, DENSE[cid], ref, 1, cid)
    _check_stream(gpu_engine, tmp_path, DENSE[cid], ref, cid)
