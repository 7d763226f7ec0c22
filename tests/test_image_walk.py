"""The walk of a ZKU1 proof on the device (zkh_image_proof_walk; include/zkhal.h "THE UPDATE'S PROOF"), what can be held to without a GPU:
the library exports the call, the header declares it, hal.py binds it with its five arguments, and the two wrappers refuse what they can
before the library is reached.  The walk itself: tests/test_image_walk_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from zeth_amd import hal as zhal
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPE = "const char* zkh_image_proof_walk(zkh_ctx*, const zkh_buf* proof, size_t words, const uint32_t root_before[8], uint32_t root_after[8]);"


def test_the_library_exports_the_walk():
    lib = C.CDLL(zhal.LIB_PATH)
    assert hasattr(lib, "zkh_image_proof_walk") and hasattr(lib, "zkh_image_proof_verify")


def test_the_header_declares_it_next_to_the_host_verifier():
    with open(os.path.join(ROOT, "include", "zkhal.h")) as fh:
        header = fh.read()
    assert PROTOTYPE in header
    verify = header.index("const char* zkh_image_proof_verify(")
    assert header.index(PROTOTYPE) == header.index("\n", verify) + 1
    assert re.search(r"zkh_image_proof_walk is the same walk ON THE DEVICE", header)


def test_the_ctypes_table_has_it_with_five_arguments():
    res, args = zhal.ABI["zkh_image_proof_walk"]
    assert res is zhal.ABI["zkh_image_proof_verify"][0] and len(args) == 5
    assert args[2] is C.c_size_t and args[3] is args[4] is zhal.ABI["zkh_image_proof_verify"][1][2]
    assert getattr(zhal.load_library(), "zkh_image_proof_walk").argtypes == args


@pytest.mark.parametrize("size", [0, 7, 9])
def test_the_wrapper_refuses_a_root_before_that_is_not_8_words(size):
    """before the library is called: no context, no GPU (the instance is never touched)"""
    nobody = object.__new__(zhal.HipHal)
    with pytest.raises(HalError, match=f"image_proof_walk: root_before of {size} words"):
        zhal.HipHal.image_proof_walk(nobody, np.zeros(12, dtype=np.uint32), np.zeros(size, dtype=np.uint32))


def test_the_prover_refuses_a_walk_without_a_proof():
    nobody = object.__new__(SegmentProver)
    seg = Segment(index=0, po2=8, zk_cycles=40, noise_seed=1)
    with pytest.raises(HalError, match="walk=True needs proof=True"):
        SegmentProver.page_out(nobody, seg, None, None, tree=object(), walk=True)
    with pytest.raises(HalError, match="walk=True needs proof=True"):
        SegmentProver.page_out(nobody, seg, None, None, walk=True)
    with pytest.raises(HalError, match="proof=True needs the image's committed tree"):
        SegmentProver.page_out(nobody, seg, None, None, proof=True, walk=True)
