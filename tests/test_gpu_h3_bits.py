"""The f16x3 forward computes, bit for bit, what it computed when tests/golden/g19_h3_bits.json was
recorded (tests/h3_bits.py --record, at the commit before the 16x16x32 tile loop's handling of
the row exponents was rearranged: the combined exponents kept in the stage rows' padding through
the K loop instead of gathered twice, one atomicMax per output row and workgroup instead of one
per wave).  Predictions, x0 and every hidden slice, and every row-exponent slot, at the lane
counts that reach each tile (tests/h3_bits.py), with rows at the exponent clamps, non-finite rows,
rows 1e4 x and 1e-4 x the scale and rows whose largest slice is the last."""
import json
import os

import pytest

import h3_bits

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "g19_h3_bits.json")


@pytest.fixture(scope="module")
def recorded():
    assert os.path.exists(FIXTURE), f"{FIXTURE} is missing (record it with tests/h3_bits.py --record)"
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tensors():
    return h3_bits.runs()


def test_same_tensors(recorded, tensors):
    assert sorted(tensors) == sorted(recorded)


@pytest.mark.parametrize("case", [c[0] for c in h3_bits.CASES])
def test_rows_cover_the_exponent_cases(tensors, case):
    """Slots at both clamps (zero slices; inf / NaN rows) and rows led by the last slice."""
    cls = h3_bits.row_classes(tensors[f"{case}.rexp"])
    print(case, cls)
    assert cls["clamp_lo"] > 0 and cls["clamp_hi"] > 0 and cls["last_max"] > 0, cls


@pytest.mark.parametrize("case", [c[0] for c in h3_bits.CASES])
def test_bits(recorded, tensors, case):
    bad = []
    for n in (f"{case}.preds", f"{case}.act", f"{case}.rexp"):
        if h3_bits.digest(tensors[n]) != recorded[n]["sha256"]:
            print(f"{n}: finite sum {h3_bits.finite_sum(tensors[n])!r} (recorded {recorded[n]['finite_sum']!r})")
            bad.append(n)
    assert not bad, f"{bad} differ from the recording"
