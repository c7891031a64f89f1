"""The plan of a recurrence launch (rnn_plan.hip plan_rec), both directions of
time and every version, through the test hook kctc_test_rec_plan.  Nothing is
launched.  The table was recorded from the build before plan_rec existed
(profiles/r10_parent_rec_plan.txt: the trace header and the kernel trace of one
T = 12 forward + backward-data per shape on an MI355X with all 256 CUs, and
that build's LDS-size and XCD-mask functions run for the same shapes); a
change to the selection has to change this table too."""
import ctypes

import pytest

from test_rec6_select_gpu import BF16, GRU, LSTM, RELU, TANH, X3, _select

pytestmark = pytest.mark.gpu


def _plan(kctc, mode, prec, H, N, fwd, dirs=2):
    out = (ctypes.c_long * 8)()
    assert kctc.lib().kctc_test_rec_plan(mode, prec, H, dirs, N, int(fwd), out) == 0
    return tuple(out)


@pytest.fixture
def whole_chip(kctc, gpu):
    """The plans below are those of a whole chip (workgroups within the usable CUs, XCD pinning)."""
    import torch
    usable = _select(kctc, LSTM, X3, 512, 16, True)[2]
    if usable != 256 or torch.cuda.get_device_properties(gpu).multi_processor_count != 256:
        pytest.skip("needs all 256 CUs usable and no CU budget")


# (mode, prec, H, N) -> forward and backward (version, U, grid, threads, LDS bytes, XCD mask, nwg, xpd)
PLANS = [
    # the LSTM rows of test_rec6_select_gpu.TABLE
    ((LSTM, X3, 512, 8), (6, 16, 256, 512, 98304, 0x3, 32, 1), (6, 16, 256, 512, 98304, 0x3, 32, 1)),
    ((LSTM, X3, 512, 16), (6, 16, 256, 512, 98304, 0xF, 32, 1), (6, 16, 256, 512, 98304, 0xF, 32, 1)),
    ((LSTM, X3, 512, 32), (6, 16, 256, 512, 98304, 0xF, 32, 1), (6, 16, 256, 512, 98304, 0xF, 32, 1)),
    ((LSTM, X3, 512, 64), (6, 32, 128, 512, 98304, 0xFF, 16, 1), (6, 32, 128, 512, 98304, 0xFF, 16, 1)),  # configs[2]
    ((LSTM, BF16, 512, 16), (6, 16, 256, 512, 98304, 0xF, 32, 1), (6, 16, 256, 512, 98304, 0xF, 32, 1)),
    ((LSTM, X3, 256, 16), (6, 16, 128, 256, 98304, 0xF, 16, 1), (6, 16, 128, 256, 98304, 0xF, 16, 1)),
    ((GRU, BF16, 1024, 32), (6, 32, 256, 512, 98304, 0xF, 32, 1), (6, 32, 256, 512, 98304, 0xF, 32, 1)),  # configs[4]
    # v4: the shapes v6 does not compile
    ((RELU, X3, 32, 4), (4, 8, 32, 256, 6400, 0, 4, 1), (4, 16, 16, 256, 6400, 0, 2, 1)),
    ((RELU, X3, 256, 16), (4, 8, 256, 256, 20736, 0, 32, 1), (4, 16, 128, 256, 20736, 0, 16, 1)),
    ((TANH, X3, 32, 4), (4, 8, 32, 256, 6400, 0, 4, 1), (4, 16, 16, 256, 6400, 0, 2, 1)),
    ((TANH, X3, 256, 16), (4, 8, 256, 256, 20736, 0, 32, 1), (4, 16, 128, 256, 20736, 0, 16, 1)),
    ((LSTM, X3, 384, 16), (4, 16, 192, 256, 115712, 0, 24, 1), (4, 16, 192, 256, 106752, 0, 24, 1)),
    # the same kernels in plain block mapping (xpd 0): no U gives a direction whole XCD slots
    ((TANH, X3, 1536, 16), (4, 16, 192, 256, 102656, 0, 96, 0), (4, 16, 192, 256, 102656, 0, 96, 0)),
    ((TANH, X3, 528, 2), (4, 8, 132, 256, 38144, 0, 66, 0), (4, 16, 66, 256, 38144, 0, 33, 0)),
    # ... and no whole-slot U whose backward image (U rows of R^T) fits the LDS
    ((LSTM, X3, 640, 2), (4, 8, 160, 256, 90624, 0, 80, 0), (4, 8, 160, 256, 86144, 0, 80, 0)),
    # not supported: bf16 exists on v6 only
    ((LSTM, BF16, 384, 16), (0,) * 8, (0,) * 8),
]


@pytest.mark.parametrize("shape,fwd_plan,bwd_plan", PLANS, ids=["m%d_p%d_H%d_N%d" % p[0] for p in PLANS])
def test_plan_table(kctc, whole_chip, monkeypatch, shape, fwd_plan, bwd_plan):
    for var in ("KCTC_STK", "KCTC_STK_FWD", "KCTC_REC_GS", "KCTC_XCD6", "KCTC_XCD6F"):
        monkeypatch.delenv(var, raising=False)
    assert _plan(kctc, *shape, True) == fwd_plan
    assert _plan(kctc, *shape, False) == bwd_plan


def test_unpinned_plan(kctc, whole_chip, monkeypatch):
    """KCTC_XCD6F=0 / KCTC_XCD6=0: no XCD mask, one workgroup per (row group, direction, unit slice)."""
    monkeypatch.setenv("KCTC_XCD6F", "0")
    monkeypatch.setenv("KCTC_XCD6", "0")
    for fwd in (True, False):
        assert _plan(kctc, LSTM, X3, 512, 16, fwd) == (6, 16, 128, 512, 98304, 0, 32, 0)
