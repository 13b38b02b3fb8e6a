"""CPU-only: which of two simultaneous faults the preconditioned group
libraries' solve_device reports (lib/libhpccg_hip_{pcg,srcg,poly,poly32}_group.so).
The four share their argument checks (csrc/hpccg_group_host.h); the message a
caller reads for a given set of bad arguments is behaviour, and the group pcg
and srcg differ from the polynomial units in one place: those look at Ms[r]
beside B_dev[r] and X_dev[r], before the degree; these leave a NULL handle to
the group's check, after every array. Fake handles, as in each library's
test_bad_arguments_are_refused_without_a_device: every call here is refused
before a handle is dereferenced. No device, no matrix.
"""
import ctypes as C

import pytest

EINVAL = -1

# library -> (message prefix, whether solve_device takes degree, lmin, lmax)
UNITS = {"pcg_group": ("group pcg", False), "srcg_group": ("group srcg", False), "poly_group": ("group poly", True),
         "poly32_group": ("group poly32", True), "srpoly_group": ("group srpoly", True)}
POLY = [u for u, (_, poly) in UNITS.items() if poly]

buf = (C.c_double * 8)()
p = C.addressof(buf)


def refused(hp, unit, Ms=(p, p), nrhs=2, b=(p, p), ldb=(4, 4), x=(p, p), minv=None, degree=2):
    """The message of a refused solve_device of two members (NULL: None)."""
    who, poly = UNITS[unit]
    fn = getattr(getattr(hp, unit + "_lib")(), f"hpccg_hip_{who.replace(' ', '_')}_solve_device")
    ptrs = lambda v: None if v is None else (C.c_void_p * 2)(*v)
    it, nr, ld = (C.c_int * 4)(), (C.c_double * 4)(), (C.c_longlong * 2)(4, 4)
    rest = (degree, 0.0, 0.0) if poly else ()
    rc = fn(ptrs(Ms), 2, nrhs, ptrs(b), None if ldb is None else (C.c_longlong * 2)(*ldb), ptrs(x), ld, ptrs(minv),
            *rest, 10, 0.0, it, nr, None)
    assert rc == EINVAL
    return hp.lib().hpccg_hip_last_error().decode()


@pytest.mark.parametrize("unit", UNITS)
def test_nrhs_comes_before_a_null_array(hp, unit):
    assert refused(hp, unit, nrhs=0, ldb=None) == f"{UNITS[unit][0]}: nrhs 0 (at least 1)"


@pytest.mark.parametrize("unit", UNITS)
def test_a_member_s_minv_comes_before_a_later_member_s_columns(hp, unit):
    assert refused(hp, unit, b=(p, None), minv=(None, p)) == f"{UNITS[unit][0]}: minv_dev[0] is NULL"


@pytest.mark.parametrize("unit", UNITS)
def test_a_null_handle_against_a_null_column(hp, unit):
    who, poly = UNITS[unit]
    # the polynomial units look at Ms[r] in the loop over the members; pcg and
    # srcg leave it to the group's check, which follows every array
    want = f"{who}: Ms[0] is NULL" if poly else f"{who}: B_dev[1] or X_dev[1] is NULL"
    assert refused(hp, unit, Ms=(None, p), x=(p, None)) == want


@pytest.mark.parametrize("unit", POLY)
def test_a_null_handle_comes_before_the_degree(hp, unit):
    assert refused(hp, unit, Ms=(p, None), degree=99) == f"{UNITS[unit][0]}: Ms[1] is NULL"
