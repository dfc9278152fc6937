"""The batch planner of DynamicsEnsemble.train_on_device against real DataLoaders (no GPU).

DynamicsModel.train (milo/milo/dynamics.py:305-378) iterates DataLoader(shuffle=True) objects
that draw from torch's global generator, member-major, a validation iteration after every
train epoch under `validate`.  plan_batches / materialise must give the same index batches for
every (member, epoch[, val]) and leave the generator in the same state."""
import pytest
import torch
from torch.utils.data import DataLoader

from amp_extensions_amd.datasets import AmpDataset
from amp_extensions_amd.ensemble import index_loader, materialise, plan_batches

S, A = 3, 2

CASES = [  # n, n_val, batch, epochs, M, validate
    (10, 7, 4, 2, 2, True),
    (37, 0, 8, 3, 4, False),
    (64, 20, 64, 1, 3, True),
    (5, 5, 1, 2, 1, True),
    (300, 90, 256, 2, 4, True),
]


def _dataset(n, tag):
    """Rows that carry their own index in column 0."""
    s = torch.arange(n, dtype=torch.float32)[:, None].repeat(1, S) + tag
    return AmpDataset(s, torch.zeros(n, A), s + 1)


def _indices(loader, tag):
    return [[int(round(float(v) - tag)) for v in state[:, 0]] for state, _, _ in loader]


@pytest.mark.parametrize("n,n_val,batch,epochs,M,validate", CASES)
def test_planner_matches_dataloaders(n, n_val, batch, epochs, M, validate):
    # the reference: one shared loader per split, iterated member-major from the global generator
    torch.manual_seed(1234)
    train = DataLoader(_dataset(n, 0.0), batch_size=batch, shuffle=True)
    val = DataLoader(_dataset(n_val, 1000.0), batch_size=batch, shuffle=True) if validate else None
    want = []
    for _ in range(M):
        rows = []
        for _ in range(epochs):
            t = _indices(train, 0.0)
            rows.append((t, _indices(val, 1000.0) if validate else None))
        want.append(rows)
    want_state = torch.get_rng_state()

    torch.manual_seed(1234)
    plan, final = plan_batches(n, n_val, batch, epochs, M, validate)
    assert torch.equal(torch.get_rng_state(), want_state)
    assert torch.equal(final, want_state)
    tl, vl = index_loader(n, batch), (index_loader(n_val, batch) if validate else None)
    # any order of materialisation (the lock-step loop goes epoch-major)
    for e in reversed(range(epochs)):
        for g in range(M):
            st, sv = plan[g][e]
            got = materialise(tl, st)
            assert got == want[g][e][0], (g, e)
            assert [len(b) for b in got] == [batch] * (n // batch) + ([n % batch] if n % batch else [])
            if validate:
                assert materialise(vl, sv) == want[g][e][1], (g, e, "val")
            else:
                assert sv is None


def test_train_still_raises_and_names_the_method():
    """DynamicsEnsemble.train / DynamicsModel.train keep raising (a pinned GPU test requires
    it); the message names train_on_device."""
    from amp_extensions_amd.ensemble import DynamicsEnsemble, DynamicsModel
    assert callable(DynamicsEnsemble.train_on_device) and callable(DynamicsEnsemble.sync_to_host)
    for cls in (DynamicsEnsemble, DynamicsModel):
        with pytest.raises(NotImplementedError, match="train_on_device"):
            cls.train(object.__new__(cls), 1)
