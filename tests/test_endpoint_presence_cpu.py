"""The endpoint presence words without a GPU: csrc/presence_rule.h -- when a table keeps words, when a domain may
read them, and the funnel that shifts them to the domain -- in a stand-alone host program under ASan + UBSan
(tests/sanitize/presence_san.cpp) against Python integers, and the resources of the kernels around hop 1 read
from the built gfx950 code object."""
import os
import re

import pytest

from test_narrow_endpoints_cpu import LLVM, OBJ, _kernels
from test_sanitizers import ASAN, SAN, _build, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cypher-for-apache-spark_amd", "csrc")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
# presence_san.cpp's table words
WORDS = [0x9E3779B9 | 0x80000001, 0x7F4A7C15 | 0x80000001, 0xF39CC060 | 0x80000001]


@pytest.fixture(scope="module")
def san(tmp_path_factory):
    d = tmp_path_factory.mktemp("presence_san")
    exe = str(d / "presence_san")
    _build(["g++", *ASAN, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(SAN, "presence_san.cpp"), "-o", exe], d)
    return lambda *args: _run(exe, *[str(a) for a in args]).split()


def test_presence_word_against_integers(san):
    """every shift 0 .. 63, word counts 1, 2 and 3, every w from one below to beyond one above the range: the
    table's bits as one integer, shifted, cut into 32-bit words"""
    out = san("word")
    seen = 0
    for nw, shift, w, v in zip(*[iter(out)] * 4):
        nw, shift, w, v = int(nw), int(shift), int(w), int(v)
        bits = sum(x << (32 * k) for k, x in enumerate(WORDS[:nw])) << shift
        want = (bits >> (32 * w)) & 0xFFFFFFFF if w >= 0 else 0
        assert v == want, (nw, shift, w, hex(v), hex(want))
        seen += 1
    assert seen == sum(64 * (nw + 5) for nw in (1, 2, 3))
    # the range's last word holds bits, the one above it none
    one = {(int(a), int(b), int(c)): int(d) for a, b, c, d in zip(*[iter(out)] * 4)}
    assert one[3, 63, 4] != 0 and one[3, 63, 5] == 0 and one[1, 0, 0] == WORDS[0] and one[1, 0, 1] == 0


def _eligible(lo, hi, rows=5, sv=0, dv=0):
    """the rule in exact integers: one bit per id from lo to the largest id the window admits, at most 2^26"""
    if sv or dv or rows <= 0 or hi <= lo:
        return False
    top = hi if hi == I64_MAX else hi - 1  # hi = INT64_MAX may stand for a maximum of INT64_MAX itself
    return top - lo + 1 <= 1 << 26


ELIGIBLE = [
    (0, 1 << 26), (0, (1 << 26) + 1), (0, (1 << 26) - 1), (0, 1), (5, 5), (7, 3),
    (-(1 << 25), 1 << 25), (-(1 << 25) - 1, 1 << 25), (-5000, 77), (-(1 << 26), 0), (-(1 << 26) - 1, 0),
    (I64_MIN, I64_MIN + (1 << 26)), (I64_MIN, I64_MIN + (1 << 26) + 1), (I64_MIN, I64_MAX), (I64_MIN, 0), (-1, I64_MAX),
    (I64_MAX - (1 << 26), I64_MAX), (I64_MAX - (1 << 26) + 1, I64_MAX), (I64_MAX - 1, I64_MAX),
    (I64_MAX - (1 << 26) - 1, I64_MAX - 1), (I64_MAX - (1 << 26) - 2, I64_MAX - 1),
    ((1 << 40) + 12345, (1 << 40) + 12345 + (1 << 26)),
]


def test_presence_eligible_at_window_edges(san):
    flat = [x for lo, hi in ELIGIBLE for x in (lo, hi, 5, 0, 0)]
    flat += [0, 100, 0, 0, 0, 0, 100, 5, 1, 0, 0, 100, 5, 0, 1, 0, 100, 1, 0, 0]
    got = [v == "1" for v in san("eligible", *flat)]
    want = [_eligible(lo, hi) for lo, hi in ELIGIBLE] + [False, False, False, True]
    assert got == want
    named = dict(zip(ELIGIBLE, got))
    assert named[0, 1 << 26] and not named[0, (1 << 26) + 1]                       # a span of 2^26 ids, and one more
    assert named[-(1 << 25), 1 << 25] and not named[-(1 << 25) - 1, 1 << 25]       # a negative lo
    assert named[I64_MAX - (1 << 26) + 1, I64_MAX] and not named[I64_MAX - (1 << 26), I64_MAX]  # hi = INT64_MAX
    assert not named[I64_MIN, I64_MAX]                                            # 2^64 - 1, not an overflow


def test_presence_usable(san):
    cases = {(10, 20, 10, 20): True,    # equal
             (12, 18, 10, 20): True,    # inner
             (10, 15, 10, 20): True, (15, 20, 10, 20): True,     # touching either end from inside
             (19, 20, 10, 20): True,    # the single last id
             (9, 20, 10, 20): False, (10, 21, 10, 20): False,    # overhanging by one id
             (0, 10, 10, 20): False, (20, 30, 10, 20): False,    # touching from outside
             (-5, 5, -10, 10): True, (-11, 5, -10, 10): False,
             (I64_MIN, I64_MIN + 5, I64_MIN, I64_MAX): True, (I64_MAX - 5, I64_MAX, 0, I64_MAX): True}
    got = [v == "1" for v in san("usable", *[x for k in cases for x in k])]
    assert got == list(cases.values())


# vgpr_count of the kernels that run beside hop 1, as the parent commit's build has them: the new kernel and the
# host code around it share their file
PASS1 = {"k_scatter_cILi1024ELi8ELi4ELb0ELb0EjE": 108, "k_scatter_cILi1024ELi8ELi4ELb0ELb0ElE": 126,
         "k_scatter_cILi1024ELi8ELi4ELb0ELb1EjE": 121, "k_scatter_cILi1024ELi8ELi4ELb0ELb1ElE": 128,
         "k_scatter_lILi1024ELi8ELi4ELb0ELb0ELb0ELb0EjE": 111, "k_scatter_lILi1024ELi8ELi4ELb0ELb0ELb0ELb0ElE": 128,
         "k_scatter_lILi1024ELi8ELi4ELb0ELb1ELb0ELb0EjE": 113, "k_scatter_lILi1024ELi8ELi4ELb0ELb1ELb0ELb0ElE": 128,
         "k_scatter_lILi1024ELi8ELi4ELb1ELb0ELb0ELb0EjE": 103, "k_scatter_lILi1024ELi8ELi4ELb1ELb0ELb0ELb0ElE": 123}
HOP2 = {"k_pool_hop2ILb1ELi0EE": 112, "k_pool_hop2ILb1ELi1EE": 128}  # over the split pool: plain, with the exchange


@pytest.mark.skipif(not os.path.exists(OBJ) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")),
                    reason="k_part.o not built or no ROCm llvm tools")
def test_kernel_resources(tmp_path):
    ks = _kernels(OBJ, str(tmp_path))
    new = [v for k, v in ks.items() if "k_presence_hop1" in k]
    assert len(new) == 1 and new[0][1] == 0 and new[0][0] <= 32, new  # no scratch; a streaming kernel's registers
    for part, vgprs in {**PASS1, **HOP2}.items():
        hit = [v for k, v in ks.items() if re.search(r"\d" + re.escape(part) + "Ev", k)]
        assert len(hit) == 1, (part, hit)
        assert hit[0] == (vgprs, 0), (part, hit[0])
