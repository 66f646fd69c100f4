"""The DEVICE build of csrc/swd_libm.h (exp, log1p) and of the composites the quaternary decoder puts on top of it (bp4_log1pexp /
bp4_logaddexp of csrc/swd_bp4_kernel.h, branch-free; the general form's called copies of csrc/swd_huge_bp4.hip) against the HOST
build of the same header under the reference's if/else composites (tests/csrc/libm_check.c), argument by argument and bit for bit,
through the diagnostic entry point swd_diag_libm.  The arguments (tests/libm_args.py) sit on every branch of the code -- whole decodes
reach exp and log1p with arguments of ordinary size only -- and are the ones tests/test_libm_restatement.py holds the host build to
the C library on: device == header == C library on one argument set.  Two NaNs are equal whatever their payload (the device's
default NaN is not x86's); every other value, +-0 included, is compared by bits."""
import numpy as np
import pytest

from tests import libm_args as A

pytestmark = pytest.mark.gpu

OP_NAMES = {0: "swd_exp", 1: "swd_exp_from(LDS table)", 2: "swd_log1p", 3: "bp4_log1pexp", 4: "bp4_logaddexp", 5: "hb_log1pexp",
            6: "hb_logaddexp"}


@pytest.mark.parametrize("op", sorted(OP_NAMES))
def test_device_equals_host_header(op):
    from slidingwindowdecoder_amd.decoders import diag_libm
    x, y = A.args(op)
    want = A.host_evaluator()("header", op, x, y)
    got = diag_libm(op, x, y)
    assert got.shape == x.shape and got.dtype == np.float64
    bad = A.differing(got, want)
    if bad.size:
        msg = A.report(OP_NAMES[op], bad, x, y, got, want)
        print(msg)
        pytest.fail(msg)


def test_tensor_in_tensor_out_and_refusals():
    """the wrapper returns what it was given (CUDA tensors stay on the device), an empty array is a no-op, a bad op is refused"""
    import torch
    from slidingwindowdecoder_amd.decoders import diag_libm
    x = torch.tensor([0.0, 1.0, -745.2, float("inf")], dtype=torch.float64, device="cuda")
    r = diag_libm(0, x)
    assert isinstance(r, torch.Tensor) and r.is_cuda
    assert A.differing(r.cpu().numpy(), A.host_evaluator()("header", 0, x.cpu().numpy())).size == 0
    assert diag_libm(2, np.zeros(0)).shape == (0,)
    with pytest.raises(ValueError):
        diag_libm(7, np.zeros(4))
    with pytest.raises(ValueError):
        diag_libm(4, np.zeros(4))
