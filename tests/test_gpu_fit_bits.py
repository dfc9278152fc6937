"""The four device fits and the three 64 x 64 f32 products compute, bit for bit, what they computed
when tests/golden/g18_fit_bits.npz was recorded (tests/fit_bits.py --record, at the commit before
the fits' optimizer arithmetic and the products were gathered into amx_optim.* / amx_gemm64.hip).

The tolerance suites (test_gpu_vfit / efit / dfit / bcfit.py) say that the fits are right; this
one says that a change meant to leave the arithmetic alone left it alone.  A change of compiler
or device libraries that moves expf, tanhf or pow moves these digests: DESIGN.md §4 says how the
fixture is then re-recorded.  The fixture's fp64 sum, max |x| and first values of every tensor
are printed on a mismatch, beside the run's."""
import os

import numpy as np
import pytest

import fit_bits

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "g18_fit_bits.npz")


@pytest.fixture(scope="module")
def recorded():
    assert os.path.exists(FIXTURE), f"{FIXTURE} is missing (record it with tests/fit_bits.py --record)"
    g = np.load(FIXTURE)
    return {str(n): i for i, n in enumerate(g["names"])}, g


@pytest.fixture(scope="module")
def tensors():
    return fit_bits.runs()


def test_same_tensors(recorded, tensors):
    assert sorted(tensors) == sorted(recorded[0])


@pytest.mark.parametrize("group", ["vfit", "efit.a_adam_clip", "efit.c_ragged", "dfit.ls_sgd", "dfit.ls_adam",
                                   "dfit.ll_sgd", "dfit.ll_adam", "bcfit.MSE", "bcfit.MLE", "gemm"])
def test_bits(recorded, tensors, group):
    index, g = recorded
    names = [n for n in sorted(index) if n.startswith(group + ".")]
    assert names, group
    bad = []
    for n in names:
        assert n in tensors, n
        if fit_bits.digest(tensors[n]) != str(g["sha256"][index[n]]):
            s, m, head = fit_bits.summary(tensors[n])
            i = index[n]
            print(f"{n}: sum {s!r} (recorded {float(g['sum'][i])!r}) max|x| {m!r} (recorded {float(g['maxabs'][i])!r})\n"
                  f"  first values {head.tolist()}\n  recorded     {g['head'][i].tolist()}")
            bad.append(n)
    assert not bad, (f"{bad} differ from the recording (toolchain then: torch hip {g['torch_hip']}, "
                     f"hipcc {g['hipcc']})")
