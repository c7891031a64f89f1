"""Which v6 recurrence kernel runs (rnn_plan.hip pick6: V6Cfg's U, nth, rg, gs and
variant), through the test hook kctc_test_rec6_select.  Nothing is launched.
The table is the selection rule as measured on the recipe shapes
(profiles/parent_rec6_kernel_names.txt: the kernel names a trace of these
shapes shows); a change to the rule has to change this table too."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

RELU, TANH, LSTM, GRU = 0, 1, 2, 3
X3, BF16 = 0, 1
PLAIN, STACKED, IOWAVE = 1, 2, 3


def _select(kctc, mode, prec, H, N, fwd, dirs=2):
    cfg = (ctypes.c_int * 6)()
    kernel = ctypes.c_void_p()
    rc = kctc.lib().kctc_test_rec6_select(mode, prec, H, dirs, N, int(fwd), cfg, ctypes.byref(kernel))
    assert rc == 0
    return tuple(cfg[:5]), kernel.value, cfg[5]


@pytest.fixture
def whole_chip(kctc, gpu):
    """pick6 keeps the workgroups within the CUs this process may use."""
    import torch
    usable = _select(kctc, LSTM, X3, 512, 16, True)[2]
    if usable != 256 or torch.cuda.get_device_properties(gpu).multi_processor_count != 256:
        pytest.skip("needs all 256 CUs usable and no CU budget")


# LSTM, 2 directions, default environment: (prec, H, N) -> U, nth, rg, gs, forward, backward
TABLE = [
    (X3, 512, 8, (16, 512, 1, 16), IOWAVE, PLAIN),
    (X3, 512, 16, (16, 512, 2, 8), STACKED, STACKED),
    (X3, 512, 32, (16, 512, 2, 16), IOWAVE, PLAIN),
    (X3, 512, 64, (32, 512, 4, 16), PLAIN, PLAIN),
    (BF16, 512, 16, (16, 512, 2, 8), IOWAVE, PLAIN),
    (X3, 256, 16, (16, 256, 2, 8), PLAIN, PLAIN),
]
# at x3 / H = 512 / N = 16: environment -> U, nth, rg, gs, forward, backward
KNOBS = [
    ({"KCTC_STK_FWD": "0"}, (16, 512, 2, 8), IOWAVE, STACKED),
    ({"KCTC_STK": "0"}, (16, 512, 2, 8), IOWAVE, PLAIN),
    ({"KCTC_REC_GS": "16"}, (16, 512, 1, 16), IOWAVE, PLAIN),
]


def _check(kctc, prec, H, N, shape, fwd_variant, bwd_variant, kernels):
    for fwd, variant in ((True, fwd_variant), (False, bwd_variant)):
        cfg, kernel, _ = _select(kctc, LSTM, prec, H, N, fwd)
        assert cfg == shape + (variant,), (prec, H, N, fwd, cfg)
        assert kernel, (prec, H, N, fwd)
        kernels.setdefault((fwd, prec, H) + shape[:2] + (variant,), set()).add(kernel)


def test_selection_table(kctc, whole_chip, monkeypatch):
    for var in ("KCTC_STK", "KCTC_STK_FWD", "KCTC_REC_GS"):
        monkeypatch.delenv(var, raising=False)
    kernels = {}  # template arguments (direction, P, H, U, NTH) -> addresses the lookup returned
    for prec, H, N, shape, fv, bv in TABLE:
        _check(kctc, prec, H, N, shape, fv, bv, kernels)
    for env, shape, fv, bv in KNOBS:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            _check(kctc, X3, 512, 16, shape, fv, bv, kernels)
    # the lookup follows the variant: one kernel per set of template arguments,
    # another one for every other set
    assert all(len(v) == 1 for v in kernels.values()), kernels
    assert len({next(iter(v)) for v in kernels.values()}) == len(kernels), kernels


@pytest.mark.parametrize("mode,H", [(TANH, 256), (TANH, 512), (TANH, 384), (LSTM, 384)])
def test_not_v6(kctc, whole_chip, mode, H):
    for fwd in (True, False):
        cfg, kernel, _ = _select(kctc, mode, X3, H, 16, fwd)
        assert cfg == (0, 0, 0, 0, 0) and not kernel
