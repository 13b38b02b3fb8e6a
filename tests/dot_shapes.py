"""Problem sizes at which a dot product's completion changes shape -- a helper of
tests/test_dot_shapes_cpu.py, tests/test_gpu_dot_shapes.py and
tests/test_gpu_dot_shapes_group.py, not a test.

Every dot is completed in two levels above the 512-row slice partials: groups
of 64 slice partials, then one wave over the group sums. plan(n) restates which
arms of that code a matrix of n rows takes; TABLE holds the smallest sizes that
reach each of them, as 1 x 1 x N stencils (3 entries wide) unless marked:

  name      n                      nslices  ng    there for
  g17       1025*512+37 = 524837   1026     17    first use of register b = 1; a last group of 2 slices, a last
                                                  slice of 37 rows
  g64       2097152                4096     64    exactly one full round; finalize_groups<4>'s last size
  g65       2097153                4097     65    a second round: one group of one slice of one row; <16>
  g65_27pt  128x128x129 = 2113536  4128     65    the same round under the 27-wide kernels, 32 slices in the
                                                  last group
  g256      8388608                16384    256   the last single pass of the top level; the last polled top
  g257      8388609                16385    257   a second top pass holding one group; <32>, top_sum_wave
  (g2049, 67108865 rows, group sums through global memory: see DESIGN.md section 5.)

g17 and g65 exist as a CSR with a value of its own at every entry
(values_cases.dominant, symmetric, not dyadic: its fp32 image is inexact, so
mixed and poly32 run their fp32 kernels); every other shape is generated on the
device. The columns of a shape (columns()): b uniform in (-1, 1), x0 uniform in
columns 0 and 2 and zero in column 1, and the rows of the last slice of b
multiplied by 2^8 (2^12 at g65, 2^16 at g257), so that the last slice and the
last group carry a visible share of every dot (tests/test_dot_shapes_cpu.py
measures it; TABLE's comment has the figures that chose the factors). The
preconditioner is a caller's m as columns_fuzz.precond draws it, or Jacobi
(case(name, "jacobi")). max_iter is 5 up to g65_27pt (3 at g65) and 4 from g256
on; the Chebyshev degree is 2.

A case is a dict with the keys the helpers of tests/columns_fuzz.py and
tests/test_gpu_columns_fuzz.py read (its name is "dots_<shape>_<precond>", apart
from that table's); the references are columns_fuzz.reference and its dot
orders, unchanged, cached per case (references()) and dropped by release().
"""
import collections

import numpy as np

import columns_fuzz as cf
import oracle
import values_cases as vc
from conftest import kat2_rr0

SLICE = cf.SLICE
DEGREE = 2

Plan = collections.namedtuple("Plan", "nslices ng rounds b_used b_last top_passes in_lds finalize top")


def plan(n):
    """The arms of the dot completion at n rows.

    col_dot_total (hpccg_columns.h, "for (int g0 = threadIdx.x / kWave; g0 < ng;
    g0 += kWaves * kB)": kFinThreads = 1024 threads are kWaves = 16 waves, kB = 4
    groups per wave and round, wave w in round t holds groups 64 t + w + 16 b in
    register b; "in_lds = ng <= kFinLds", kFinLds = 2048):
      rounds      trips of the g0 loop, ceil(ng / 64);
      b_used      registers b that hold a group in the first round (1: b = 0 alone);
      b_last      the same in the last round;
      in_lds      group sums in LDS (else through gsum in global memory).
    top_sum_wave (hpccg_device.h, "for (int i0 = 0; i0 < ng; i0 += kTopThreads)",
    kTopThreads = 256):
      top_passes  trips of that loop, ceil(ng / 256).
    The single solve (hpccg_kernels.hip): k_finalize takes finalize_groups<4> for
    "ng <= 4 * (kFinalizeThreads / kWave)" = 64, <16> for ng <= 256, else <32>
    (finalize); the folded completions take top_sum_polled for
    "ng <= kTopThreads" and top_sum_wave above (top)."""
    nslices = (n + SLICE - 1) // SLICE
    ng = (nslices + 63) // 64
    rounds = (ng + 63) // 64
    last = ng - 64 * (rounds - 1)
    return Plan(nslices, ng, rounds, min(4, (min(ng, 64) + 15) // 16), min(4, (last + 15) // 16), (ng + 255) // 256,
                ng <= 2048, 4 if ng <= 64 else 16 if ng <= 256 else 32, "polled" if ng <= 256 else "wave")


# name -> (dims, nslices, ng, max_iter, log2 of the last slice's factor, distinct-valued CSR,
#          the columns held to CPU references)
# The factor and max_iter are 2^8 and 5 (4 from g256 on) unless the last slice's share of some dot of some
# restatement fell below 100 x RTRANS_RTOL_1GPU with them (tests/test_dot_shapes_cpu.py; a last slice of one
# row is at the mercy of one product p_n (Ap)_n, which crosses zero as the iterations go on):
#   g65   2^8, max_iter 5: 2e-11 (pcg, column 2, p.Ap of iteration 3); 2^12: 1e-7 there; 2^16: 5e-7;
#         chosen 2^12 and max_iter 3 (two iterations: beta and the second alpha are used): 2e-4 at least;
#   g257  2^8: 2e-9 (batch, column 0); 2^12: 5e-8; chosen 2^16 with column 0 held: 2e-5 at least (column 1,
#         x0 = 0, is dominated by its last row there and loses it after one iteration: 2e-10, not held).
TABLE = {
    "g17": ((1, 1, 1025 * 512 + 37), 1026, 17, 5, 8, True, (0, 1, 2)),
    "g64": ((1, 1, 2097152), 4096, 64, 5, 8, False, ()),
    "g65": ((1, 1, 2097153), 4097, 65, 3, 12, True, (0, 1, 2)),
    "g65_27pt": ((128, 128, 129), 4128, 65, 5, 8, False, ()),
    "g256": ((1, 1, 8388608), 16384, 256, 4, 8, False, ()),
    "g257": ((1, 1, 8388609), 16385, 257, 4, 16, False, (0,)),
}
NAMES = list(TABLE)
CSR_SHAPES = [k for k, v in TABLE.items() if v[5]]
ALL_LIBS = ("batch", "mixed", "pcg", "srcg", "poly", "poly32")
# the libraries a shape is held to a CPU restatement with
REFERENCE_LIBS = {"g17": ALL_LIBS, "g65": ALL_LIBS, "g257": ("batch", "pcg", "srcg")}

# the two groups of tests/test_gpu_dot_shapes_group.py: rows per member
# (every member's last slice of b is multiplied by its shape's factor; max_iter 5)
GROUPS = {
    "csr_g65_g17": (["g65", "g17"], True, (0, 1, 2)),
    "gen_g65_g65": (["g65", "g65"], False, (0,)),
}
GROUP_LIBS = ("batch", "pcg", "srcg", "poly", "poly32")


def counts(name):
    """A group's rows per member."""
    return [nrows(k) for k in GROUPS[name][0]]


def nrows(name):
    if name in GROUPS:
        return sum(counts(name))
    nx, ny, nz = TABLE[name][0]
    return nx * ny * nz


def rr0(name):
    """r0.r0 of the device-generated stencil with x0 = 0 and b = A 1, an integer
    exact under any summation order: KAT-2 (conftest.kat2_rr0); on 1 x 1 x N it
    is 625 (N - 2) + 1352 (row sums 25 inside and 26 at the two ends)."""
    if name in GROUPS:
        return kat2_rr0(1, 1, nrows(name))
    return kat2_rr0(*TABLE[name][0])


def case(name, precond="caller"):
    """The draws of a shape (or of a group), in the form columns_fuzz's helpers read."""
    seed = 7919 * (1 + (NAMES + list(GROUPS)).index(name))
    c = {"kind": "one", "name": f"dots_{name}_{precond}", "shape": name, "scaling": "none", "s7": False,
         "max_iter": 5, "nrhs_a": 1, "nrhs": 3, "pad": 0, "early": False, "precond": precond, "col_seed": seed + 1,
         "seed": seed, "degree": DEGREE, "bounds": precond == "jacobi"}
    if name in GROUPS:
        _, csr, held = GROUPS[name]
        cnt = counts(name)
        c.update(kind="group", P=len(cnt), slabs=cnt, dims=(1, 1, sum(cnt)), csr=csr, held=held,
                 family="csr" if csr else "stencil")
        if not csr:
            c["dims"] = (1, 1, cnt[0])  # per member, as columns_fuzz reads a stencil group
    else:
        dims, _, _, max_iter, _, csr, held = TABLE[name]
        c.update(dims=dims, max_iter=max_iter, csr=csr, held=held, family="csr" if csr else "stencil")
    return c


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def release(name=None):
    """Drop what a shape has cached (everything: None), here and in columns_fuzz."""
    for store in (_cache, cf._cache):
        mine = (name, f"dots_{name}_caller", f"dots_{name}_jacobi")
        for k in [k for k in store if k[0] in mine or (name is None and (store is _cache or k[0].startswith("dots_")))]:
            del store[k]


def matrix(name):
    """The host matrix of a shape: the distinct-valued CSR, or the stencil oracle.generate restates."""
    def make():
        n = nrows(name)
        csr = GROUPS[name][1] if name in GROUPS else TABLE[name][5]
        if csr:
            return vc.dominant(1, 1, n, False, True, False, case(name)["seed"])
        dims = (1, 1, n) if name in GROUPS else TABLE[name][0]
        return oracle.generate(*dims)
    return _cached((name, "A"), make)


def columns(name):
    """(B, X0), 3 columns: the module's docstring."""
    def make():
        n = nrows(name)
        rng = np.random.default_rng(case(name)["col_seed"])
        B = rng.uniform(-1.0, 1.0, (3, n))
        X0 = rng.uniform(-1.0, 1.0, (3, n))
        X0[1] = 0.0
        s = 0
        for k in GROUPS[name][0] if name in GROUPS else [name]:
            s += nrows(k)
            B[:, s - 1 - (nrows(k) - 1) % SLICE:s] *= 2.0 ** TABLE[k][4]
        return B, X0
    return _cached((name, "cols"), make)


def run_libs(name):
    """The libraries a shape or a group is held to a restatement with. (poly at
    degree 0 is held to pcg's: the same recurrence, and the same bits --
    tests/test_dot_shapes_cpu.py.)"""
    return GROUP_LIBS if name in GROUPS else REFERENCE_LIBS.get(name, ())


def references(c, lib, degree=DEGREE, dot="seq", cache=True):
    """columns_fuzz.reference of the held columns of a case under one library."""
    name = c["shape"]

    def make():
        A = matrix(name)
        B, X0 = columns(name)
        m = cf.precond(c, A)[1]
        lmin, lmax = cf.bounds(c, A) if lib in ("poly", "poly32") else (None, None)
        return [cf.reference(lib, A, B[k], X0[k], m, degree, c["max_iter"], 0.0, dot, lmin, lmax)
                for k in c["held"]]
    if not cache:
        return make()
    return _cached((c["name"], "ref", lib, degree, dot if isinstance(dot, str) else "second"), make)


def members(name):
    """The row ranges of a group's members."""
    out, s = [], 0
    for n in counts(name):
        out.append(slice(s, s + n))
        s += n
    return out
