"""Plain reference parse of a libffm text block, for the tests of the host
parser (csrc/io/reader.cpp) and the device parser (csrc/hip/kernels_parse.hip).

Pure Python by the rules of reader.cpp's parse_libffm / parse_token; no
project native code.  Numbers go through the C library's ``strtod`` (what
``atof`` is) on the first 63 bytes of the text up to its first NUL, as
reader.cpp's ``range_atof`` does; keys come from ``hashing.std_hash``.

Rules: lines end at '\\n'; a line without '\\t' is no row; the label is the
text before the first '\\t' (1.0 when its value is > 0.0000001, else 0.0);
the tokens after it are split at single spaces, empty ones skipped; a token
without ':' is no feature; the field id is the text before the first ':',
its value truncated toward zero to int32; the feature text runs to the second
':' or, without one, to the token end with all trailing '\\r' stripped; the
value after the second ':' is never read.

Exclusions (``parse`` raises ``Unsupported``; the C++ parser's behaviour on
these is undefined or documented as unsupported):

* a field id whose value is NaN or outside [-2**31, 2**31) -- the conversion
  to int32 is undefined;
* a label or field id that ``strtod`` reads as a hexadecimal float -- the
  device parser does not recognise them.
"""
from __future__ import annotations

import ctypes
import math
import re

import numpy as np

from .hashing import std_hash

_libc = ctypes.CDLL(None)
_libc.strtod.restype = ctypes.c_double
_libc.strtod.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]

THRESHOLD = 0.0000001
_SPACE = b" \t\n\v\f\r"
# what the device parser turns into an integer on the fly; everything else
# takes its atof
_FAST_ID = re.compile(rb"^[ \t\n\v\f\r]*[+-]?([0-9]*)$")


class Unsupported(ValueError):
    """The block holds a construct this reference excludes (module docstring)."""


def c_atof(text: bytes) -> float:
    """atof of the first 63 bytes of ``text`` (range_atof); raises
    Unsupported for a hexadecimal float."""
    buf = ctypes.create_string_buffer(bytes(text[:63]))  # (NUL terminated)
    end = ctypes.c_void_p()
    v = _libc.strtod(ctypes.addressof(buf), ctypes.byref(end))
    used = (end.value or ctypes.addressof(buf)) - ctypes.addressof(buf)
    s = buf.raw[:used].lstrip(_SPACE).lstrip(b"+-")
    if s[:2].lower() == b"0x" and len(s) > 2:
        raise Unsupported("hexadecimal float %r" % bytes(text[:63]))
    return float(v)


def label_of(text: bytes) -> float:
    return 1.0 if c_atof(text) > THRESHOLD else 0.0


def field_id_of(text: bytes) -> int:
    v = c_atof(text)
    if math.isnan(v) or v < -2.0 ** 31 or v >= 2.0 ** 31:
        raise Unsupported("field id %r is no int32" % bytes(text[:63]))
    return int(v)  # (toward zero)


def id_takes_atof(text: bytes) -> bool:
    """The field id is no optionally signed decimal integer within int32: the
    device parser's atof path reads it."""
    m = _FAST_ID.match(text)
    return m is None or int(m.group(1) or b"0") > 0x7FFFFFFF


def parse(block: bytes, row_mod: int = 1) -> dict:
    """The block as a CSR dict: labels (f32), row_ptr (i32), fgid (i32), keys
    (u64), rows, features, shortest / longest row length (0 without rows),
    nnz_per_row (the rows' common length, 0 when they differ), nnz_used (the
    features of the first rows - rows % row_mod rows), and ``stats``: what
    the block exercised (for corpus coverage checks)."""
    labels, row_ptr, fgid, keys = [], [0], [], []
    st = {"lines": 0, "no_row_lines": 0, "featureless_rows": 0, "no_colon_tokens": 0,
          "empty_tokens": 0, "cr_stripped": 0, "flens": set(), "ids_atof": 0,
          "labels_pos": 0, "labels_neg": 0, "no_final_newline": False}
    n = len(block)
    p = 0
    while p < n:
        nl = block.find(b"\n", p)
        le = nl if nl >= 0 else n
        if nl < 0:
            st["no_final_newline"] = True
        line = block[p:le]
        p = le + 1
        st["lines"] += 1
        tab = line.find(b"\t")
        if tab < 0:
            st["no_row_lines"] += 1
            continue
        y = label_of(line[:tab])
        st["labels_pos" if y else "labels_neg"] += 1
        labels.append(y)
        for tok in line[tab + 1:].split(b" "):
            if not tok:
                st["empty_tokens"] += 1
                continue
            c1 = tok.find(b":")
            if c1 < 0:
                st["no_colon_tokens"] += 1
                continue
            c2 = tok.find(b":", c1 + 1)
            if c2 >= 0:
                feat = tok[c1 + 1:c2]
            else:
                feat = tok[c1 + 1:].rstrip(b"\r")
                st["cr_stripped"] += len(feat) < len(tok) - c1 - 1
            st["flens"].add(len(feat))
            st["ids_atof"] += id_takes_atof(tok[:c1])
            fgid.append(field_id_of(tok[:c1]))
            keys.append(std_hash(feat))
        st["featureless_rows"] += len(keys) == row_ptr[-1]
        row_ptr.append(len(keys))
    rows = len(labels)
    lens = np.diff(np.asarray(row_ptr, dtype=np.int64))
    lmin = int(lens.min()) if rows else 0
    lmax = int(lens.max()) if rows else 0
    return {"labels": np.asarray(labels, dtype=np.float32),
            "row_ptr": np.asarray(row_ptr, dtype=np.int32),
            "fgid": np.asarray(fgid, dtype=np.int32),
            "keys": np.asarray(keys, dtype=np.uint64),
            "rows": rows, "features": len(keys), "lmin": lmin, "lmax": lmax,
            "nnz_per_row": lmin if lmin == lmax else 0,
            "nnz_used": int(row_ptr[rows - rows % row_mod]), "stats": st}


__all__ = ["Unsupported", "THRESHOLD", "c_atof", "label_of", "field_id_of", "id_takes_atof",
           "parse"]
