"""The late start of emit33_ypar_short's d stream (csrc/emit33.h) on the GPU: the records par33_host -late kept (tests/par33_late_cases.py:
1024 random sets, limbs 4..8 at 0 / the ceiling in every pattern, sets on both sides of the guard on column 14's truncated digit, sets on
which the late start alone gives a wrong u_6) through the function by itself on raw limbs (Device.diag_limbs, op LIMB_PAR33) - parity AND
path taken must be the host's, and both paths must have run.  A few thousand sets in one small launch; the kernels that use the function
are run by tests/test_gpu_par33.py."""
import numpy as np
import pytest

import limb_cases
import par33_cases as C
import par33_late_cases as L

pytestmark = pytest.mark.gpu


def test_parity_and_path_of_the_late_start_on_raw_limbs():
    from ecloop_amd import Device
    rc, text, recs = L.run(12)  # set 11: 4096 sets, the first 1024 kept
    assert rc == 0, text[-3000:]
    s = recs["set"]
    assert (s == 11).sum() == 1024 and (s == 12).sum() == 2048 and (s == 13).sum() >= 512 and (s == 14).sum() >= 64 and len(recs) < 8192
    full = np.zeros((len(recs), limb_cases.LIMB_IN, 9), dtype=np.uint32)
    full[:, 0], full[:, 1], full[:, 2] = recs["lam"], recs["b"], recs["Y"]
    d = Device(0)
    try:
        out, flag = d.diag_limbs(C.LIMB_PAR33, full)
    finally:
        d.close()
    bad = np.nonzero((flag != recs["par"]) | (out[:, 0, 0] != recs["path"]))[0]
    assert not len(bad), (int(bad[0]), recs[bad[0]].tolist(), int(flag[bad[0]]), int(out[bad[0], 0, 0]))
    assert (out[:, 0, 0] == 1).sum() >= 256 + 64 and (out[:, 0, 0] == 0).sum() >= 256  # both paths ran on the device: sets 13 and 14 alone
    assert not out[:, 0, 1:].any() and not out[:, 1:].any()
