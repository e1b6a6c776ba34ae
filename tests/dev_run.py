"""What tests/test_dev_placement_gpu.py and tests/test_dev_stream_gpu.py share: a case of tests/dev_cases.py put on the
device with tests/dev_place.py, called through the C ABI, read back and held against the model's answer."""
import ctypes

import numpy as np

from tests import dev_place

GUARD = 512
# the guards of the three placed runs: the two plain fills, and one whose bytes are other valid base codes than either
# (0x00 is base 0, 0xFF masks to base 3 and is a no-base of a read; 01 02 01 02 ... are bases 1 and 2)
FILLS = (0x00, 0xFF, (1, 2))


def device():
    import torch
    return torch.device("cuda", 0)


def put(case, data, fill, flip=0):
    """every input and every output of the case on the device -> (input views, output views, name -> address).
    fill None: the ordinary way, every input at the start of an allocation of its own; outputs are exact-capacity views
    between canaries either way.  flip: which of its two leads a byte array gets (Case.lead)."""
    import torch
    dev = device()
    assert not set(data.inp) & set(data.outs)
    ins, outs, p = {}, {}, {}
    for name, arr in data.inp.items():
        raw = arr.reshape(-1).view(np.uint8)
        if fill is None:
            t = torch.zeros(max(raw.size, 1), dtype=torch.uint8, device=dev)
            t[:raw.size].copy_(torch.from_numpy(raw.copy()))
            ins[name], p[name] = t[:raw.size], t.data_ptr()
        else:
            ins[name] = dev_place.place(arr, case.lead(name, arr, flip), GUARD, fill, device=dev)
            p[name] = ins[name].placement.address
    for name, arr in data.outs.items():
        lead = 0 if fill is None else case.lead(name, arr, flip)
        outs[name] = dev_place.place_out(arr.nbytes, lead, GUARD, 0xA5 if fill is None else fill, device=dev)
        p[name] = outs[name].placement.address
    torch.cuda.synchronize()
    return ins, outs, p


def fetch(lib, view):
    """the bytes of a device view through kiss_hip_copy_to_host: a blocking copy on the null stream, no torch call"""
    out = np.empty(view.numel(), np.uint8)
    if out.size:
        rc = lib.kiss_hip_copy_to_host(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(view.placement.address), out.size)
        assert rc == 0, rc
    return out


def fetch_outputs(lib, out_views):
    return {name: fetch(lib, v) for name, v in out_views.items()}


def check(case, data, raw_outs, scal, where):
    """every output element by element, the return code, the returned totals and the report fields against the model"""
    for k, want in data.scal.items():
        assert scal[k] == want, "%s %s: %s is %r, the model says %r (all: %r)" % (case.id, where, k, scal[k], want, scal)
    got = {name: raw_outs[name].view(data.outs[name].dtype) for name in data.outs}
    got, want = case.normalise(got, data.host), case.normalise(data.outs, data.host)
    for name in data.outs:
        sl = case.defined(name, data.host)
        g, w = got[name][sl], want[name][sl]
        assert g.shape == w.shape, (case.id, where, name, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s %s: %s differs from the model at %d of %d elements, first at [%d]: %r, the model says %r" % (
            case.id, where, name, bad.size, w.size, int(bad[0]), g[bad[0]], w[bad[0]])


def context(case):
    import kiss_amd
    return kiss_amd.Context(max_n=case.max_n)
