"""What the GPU tests of the arguments as data share (imported the way check_bus_cases is): Montgomery words, a circuit with its
arguments, traces and an image on the device, a profiled call, a host-witness seal from pinned copies, and the refusal of a LINK witness."""
import re

import numpy as np
import pytest

from zeth_amd.circuits import logup
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver

P = 2013265921
ONE = (1 << 32) % P


def enc(x):
    return (np.asarray(x, dtype=np.uint64) % np.uint64(P) * np.uint64(ONE) % np.uint64(P)).astype(np.uint32)


def circuit(hal, desc, blob):
    c = hal.load_circuit(desc, jit=False)
    c.set_arguments(blob)
    return c


def upload(hal, code, data):
    dcode, ddata = hal.alloc_elem("code", code.size), hal.alloc_elem("data", data.size)
    dcode.write(code)
    ddata.write(data)
    return dcode, ddata


def image_buf(hal, image):
    buf = hal.alloc_elem("image", image.size)
    buf.write(np.ascontiguousarray(image, dtype=np.uint32))
    return buf


def profiled(hal, call):
    """call() with the profiler on -> {scope name: its record} of the scopes that ran"""
    hal.prof_enable(True)
    hal.prof_reset()
    call()
    prof = {r["name"]: r for r in hal.prof_get() if r["calls"]}
    hal.prof_enable(False)
    return prof


def seal_host(hal, prover, seg, code, data, out, **kw):
    """seal_host_witness from pinned copies of the traces (zkh_write_async reads pinned memory only)"""
    hcode, hdata = hal.host_alloc(code.size), hal.host_alloc(data.size)
    hcode[:] = code
    hdata[:] = data
    try:
        return prover.seal_host_witness(seg, hcode, hdata, out, **kw)
    finally:
        hal.sync()
        hal.host_free(hcode)
        hal.host_free(hdata)


def links_refused(hal, desc, blob, po2, zk, code, data, want_msg, image=None, seal=False):
    """derive_links (with an image: derive_links_paged) refuses with the reference's words and leaves the data, and the image, as they
    were; seal: nothing is sealed from that witness either"""
    code, data = np.ascontiguousarray(code).reshape(-1), np.ascontiguousarray(data).reshape(-1)
    with pytest.raises(logup.ReferenceError, match="^" + re.escape(want_msg) + "$"):
        logup.reference_links(logup.Arguments.parse(blob), po2, zk, code, data, image=image)
    c = circuit(hal, desc, blob)
    dcode, ddata = upload(hal, code, data)
    dimage = None if image is None else image_buf(hal, image)
    with pytest.raises(HalError, match=re.escape("derive_links: " + want_msg + ": the witness is refused")):
        if image is None:
            hal.derive_links(c, po2, zk, dcode, ddata)
        else:
            hal.derive_links_paged(c, po2, zk, dcode, ddata, dimage)
    assert np.array_equal(ddata.to_vec(), data) and (image is None or np.array_equal(dimage.to_vec(), image))
    if seal:
        with pytest.raises(HalError, match=re.escape(want_msg)):
            seal_host(hal, SegmentProver(hal, desc, arguments=blob), Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=0x0C05), code, data,
                      np.zeros(4, dtype=np.uint32))
