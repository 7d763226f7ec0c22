"""What the GPU tests of the arguments as data share (imported the way check_bus_cases is): Montgomery words, a circuit with its
arguments, traces on the device, and a host-witness seal from pinned copies."""
import numpy as np

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
