"""The sampler's host logic without a GPU: the admission state (sampler._Admission) driven by a
fake executor must return the sequential reference's trajectories for any lane count, member
blocking, speculation and launch-to-read-back lag; and the done-flag -> store-row arithmetic
(sampler._chunk_rows) on hand-written matrices."""
import itertools
import math

import numpy as np
import pytest

from amp_extensions_amd.sampler import _Admission, _chunk_rows


def _true_length(seed: int, R: int) -> int:
    """A trajectory's length as a function of its seed: ~15 % length 1, ~35 % short (below R / 4),
    ~30 % the horizon R, the rest uniform in [1, R]."""
    rs = np.random.RandomState(seed)
    u = rs.uniform()
    if u < 0.15:
        return 1
    if u < 0.50:
        return 1 + int(rs.randint(max(1, math.ceil(R / 4) - 1)))
    if u < 0.80:
        return R
    return 1 + int(rs.randint(R))


def _sequential(W: int, quota: int, mode: str, base_seed: int, R: int) -> list[list[int]]:
    """Per worker the lengths of trajectories 1..n_i: n_i = min{n : sum_{j <= n} len_j >= q}
    ('trajectories': the first q)."""
    out = []
    for w in range(W):
        lens = []
        for j in itertools.count(1):
            if (sum(lens) >= quota) if mode == "samples" else (len(lens) == quota):
                break
            lens.append(_true_length(12345 + base_seed * w + j, R))
        out.append(lens)
    return out


def _check_lanes(adm: _Admission, L: int, seen: list) -> None:
    """No lane is held by two trajectories; a lane is held or free, never both; every ended or
    dropped trajectory has given its lane back."""
    admitted = [tr for trs in adm.adm for tr in trs]
    held = [tr.lane for tr in admitted if tr.lane >= 0]
    assert len(held) == len(set(held))
    for tr in admitted:
        assert (tr.lane == -1) if tr.ended else (adm.lane_tr[tr.lane] is tr)
    assert sum(t is not None for t in adm.lane_tr) == len(held)
    free = [b for lst in adm.free.lists for b in lst]
    assert sorted(free + held) == list(range(L))
    kept = set(map(id, admitted))
    assert all(tr.lane == -1 for tr in seen if id(tr) not in kept)  # the dropped


def _run(adm: _Admission, L: int, K: int, lag: int) -> None:
    """The collection loop's skeleton over a fake executor: a chunk advances every live launched
    pair by min(K, remaining).  lag 0: right after the launch; lag 1: after the next launch, with
    the tail rule and the final drain."""
    R, seen = adm.R, []

    def read_back(launched):
        live = adm.live(launched)
        assert all(adm.lane_tr[b] is tr for b, tr in live)  # (never a dropped trajectory's steps)
        if live:
            rem = np.array([_true_length(tr.seed, R) - tr.length for _, tr in live])
            assert (rem > 0).all()
            adm.advance(live, np.minimum(rem, K), rem <= K, np.zeros(len(live), np.int64))
        _check_lanes(adm, L, seen)

    pending, chunks = None, 0
    while True:
        new = adm.admit()
        seen.extend(new)
        _check_lanes(adm, L, seen)
        launched = adm.in_flight()
        assert all(adm.lane_tr[tr.lane] is tr for tr in new)
        tail = pending is not None and not new and all(tr.length + K >= R for _, tr in launched)
        if not launched or tail:
            if pending is None:
                break
            read_back(pending)
            pending = None
            continue
        chunks += 1
        assert chunks <= 4 * (adm.W * adm.quota + adm.W) * (R + K) // K + 64  # the sampler's step budget
        if lag == 0:
            read_back(launched)
            continue
        if pending is not None:
            read_back(pending)
        pending = launched


CASES = [(2, 400, "samples", 40, 8), (3, 257, "samples", 25, 5), (3, 9, "trajectories", 30, 8),
         (4, 999, "samples", 60, 7), (1, 1, "samples", 5, 16)]
LANES = [(512, 4, 0), (512, 4, 128), (3, 4, 0), (8, 4, 2)]


@pytest.mark.parametrize("lag", [0, 1])
@pytest.mark.parametrize("speculate", [True, False])
@pytest.mark.parametrize("L,M,Bq", LANES)
@pytest.mark.parametrize("W,N,mode,R,K", CASES)
def test_admission_equals_sequential_reference(W, N, mode, R, K, L, M, Bq, speculate, lag):
    base_seed = 7
    quota = math.ceil(N / W)
    adm = _Admission(W, quota, mode, base_seed, R, speculate, L, M, Bq)
    _run(adm, L, K, lag)
    trajs = adm.trajectories()
    assert all(tr.ended and tr.lane == -1 for tr in trajs)
    assert [(tr.worker, tr.j) for tr in trajs] == [(w, j + 1) for w in range(W) for j in range(len(adm.adm[w]))]
    assert [tr.seed for tr in trajs] == [12345 + base_seed * tr.worker + tr.j for tr in trajs]
    assert all(sum(n for _, n in tr.segs) == tr.length for tr in trajs)
    assert [[tr.length for tr in trs] for trs in adm.adm] == _sequential(W, quota, mode, base_seed, R)
    assert not any(adm.lane_tr) and sorted(b for lst in adm.free.lists for b in lst) == list(range(L))


def test_chunk_rows_hand_written():
    """K = 4, lanes 1, 4, 6 of L = 8: lane 1 never ends, lane 4 ends at step 0 (a later flag of
    its idle steps is ignored), lane 6 at the last step."""
    lanes = np.array([1, 4, 6], np.int64)
    done = np.array([[0, 1, 0],
                     [0, 0, 0],
                     [0, 1, 0],
                     [0, 0, 1]], bool)
    n, hit, starts, flat = _chunk_rows(done, lanes, 8)
    assert n.tolist() == [4, 1, 4]
    assert hit.tolist() == [False, True, True]
    assert starts.tolist() == [0, 4, 5]
    assert flat.tolist() == [1, 9, 17, 25, 4, 6, 14, 22, 30]


def test_chunk_rows_nothing_ends():
    lanes = np.array([1, 4, 6], np.int64)
    n, hit, starts, flat = _chunk_rows(np.zeros((4, 3), bool), lanes, 8)
    assert n.tolist() == [4, 4, 4]
    assert hit.tolist() == [False, False, False]
    assert starts.tolist() == [0, 4, 8]
    assert flat.tolist() == [1, 9, 17, 25, 4, 12, 20, 28, 6, 14, 22, 30]
