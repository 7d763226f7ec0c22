"""zkh_derive_all (csrc/arguments.hip) on a GPU-less circuit: it runs the stages a blob has in the order sorted, columns, links,
multiplicities, so with a NULL context the first stage present is the one that objects; a blob that derives nothing, and a circuit
without arguments, are no-ops that look at no other argument; a NULL circuit is its only own error.  No GPU."""
import numpy as np
import pytest

from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.hal import HalError

TINY = syn_lookup.TINY


def _circuit(blob=None, **flags):
    desc, built = syn_lookup.build_syn_lookup(TINY, **flags)
    hc = zhal.HostCircuit(desc)
    if blob is None:
        blob = built
    b = np.ascontiguousarray(blob, dtype=np.uint32)
    zhal._check(zhal._lib.zkh_circuit_set_arguments(hc.h, zhal._ptr(b), b.size))
    return hc


def _derive_all(h):
    zhal._check(zhal._lib.zkh_derive_all(None, h, 8, 40, None, None))


@pytest.mark.parametrize("flags,first", [
    (dict(sort=True, limbs=True, derive=True), "derive_sorted"),
    (dict(limbs=True, derive=True), "derive_columns"),
    (dict(link=True), "derive_links"),
    (dict(derive=True), "derive_multiplicities"),
])
def test_the_first_stage_present_objects_to_a_null_context(flags, first):
    with pytest.raises(HalError, match=f"^{first}: null argument"):
        _derive_all(_circuit(**flags).h)


def test_nothing_to_derive_is_a_no_op_that_reads_no_argument():
    full = syn_lookup.build_syn_lookup(TINY, sort=True, limbs=True, derive=True)[1]
    _derive_all(_circuit(blob=logup.Arguments.parse(full).plain().blob(), sort=True, limbs=True, derive=True).h)
    hc = _circuit()                                                         # the version-1 blob: no flag anywhere
    _derive_all(hc.h)
    zhal._check(zhal._lib.zkh_circuit_set_arguments(hc.h, None, 0))           # ... and no arguments at all
    assert not zhal._lib.zkh_circuit_has_arguments(hc.h)
    _derive_all(hc.h)


def test_a_null_circuit_is_refused():
    with pytest.raises(HalError, match="^derive_all: null circuit"):
        _derive_all(None)
