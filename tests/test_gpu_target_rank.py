"""The fused target-rank kernel (csrc/retrieve.hip rs_target_rank) and the layers above it
(ops.target_rank, ItemIndex.rank / columns_of, TwoTowerModel.rank_targets, evaluate_ranking).

Definition under test: rank[b] = #{ j != t : m(b, j) > m(b, t) or (m(b, j) == m(b, t) and j < t) }
with m the history-masked score, i.e. the target's position in rs_fused_topk's order; -1 for a
target outside the catalog. Integer-valued embeddings with |x| <= 3 make every score exact in fp32
and in bf16, so ranks are compared for equality with numpy on float64 scores, for the automatic and
the forced splits and both item dtypes. On real-valued data the expected rank is the target's
position in the pre-existing ops.fused_topk's list, which must hold bit-exact ties included."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from recommendsystemproject_amd import ops  # noqa: E402
from recommendsystemproject_amd.project.utils.training_utils import (evaluate_ranking, to_device,  # noqa: E402
                                                                      validate)
from recommendsystemproject_amd.retrieval import ItemIndex, sorted_history_csr  # noqa: E402
from test_gpu_fused_retrieval import _demo_model  # noqa: E402
from test_gpu_retrieval import _history, _mask_reference  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}


def _dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def np_rank(S, tcols):
    """The definition, on masked scores S [B, N]."""
    B, N = S.shape
    out = np.full(B, -1, np.int64)
    cols = np.arange(N)
    for b, t in enumerate(tcols):
        if 0 <= t < N:
            out[b] = int((S[b] > S[b, t]).sum() + ((S[b] == S[b, t]) & (cols < t)).sum())
    return out


def _hist_cols(hist, u, N):
    """The catalog columns (item id - 100) of user u's history, ascending."""
    return np.array(sorted(x - 100 for x in hist.get(int(u), ()) if 100 <= x < 100 + N), dtype=np.int64)


def _targets(rng, B, N):
    """Random columns, with column 0, column N - 1, -1, N and one column shared by three users."""
    t = rng.integers(0, N, B)
    special = [0, N - 1, -1, N, N // 2, N // 2, N // 2]
    t[:min(B, len(special))] = special[:B]
    return t.astype(np.int32)


def _check_exact(Ue, Ie, tcols, dtype, S=None, users=None, hist=None):
    """target_rank == np_rank(S) for the automatic and the forced splits."""
    if S is None:
        S = Ue.astype(np.float64) @ Ie.astype(np.float64).T
    want = np_rank(S, tcols)
    U, I, T = _dev(Ue), _dev(Ie, DTYPES[dtype]), _dev(tcols)
    u_dev = _dev(users) if users is not None else None
    for splits in [0] + [s for s in (1, 3, 8) if Ie.shape[0] // s >= 1]:
        got = ops.target_rank(U, I, T, u_dev, hist, splits=splits)
        assert got.dtype == torch.int32 and got.shape == (Ue.shape[0],)
        assert np.array_equal(got.cpu().numpy(), want), (dtype, splits)
    return want


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('B,N,D', [(1, 1, 16), (37, 7, 16), (129, 1000, 64), (150, 2100, 80), (150, 2100, 144),
                                   (48, 5000, 128), (33, 70001, 128), (19, 4096, 256)])
def test_shapes(B, N, D, dtype):
    """A partial row tile, more than one row tile, widths that are not an instance's built size, a
    last column tile that is not full, more than one automatic split (70001 columns)."""
    rng = np.random.default_rng(B + N + D)
    Ue = rng.integers(-3, 4, (B, D)).astype(np.float32)
    Ie = rng.integers(-3, 4, (N, D)).astype(np.float32)
    tcols = _targets(rng, B, N)
    want = _check_exact(Ue, Ie, tcols, dtype)
    assert all(want[i] == -1 for i in (2, 3) if i < B)
    # any integer dtype of target columns, and a strided view of them
    wide = _dev(np.stack([tcols.astype(np.int64), np.zeros(B, np.int64)], axis=1))[:, 0]
    assert np.array_equal(ops.target_rank(_dev(Ue), _dev(Ie, DTYPES[dtype]), wide).cpu().numpy(), want)


def test_automatic_splits_cover_the_large_shape():
    from recommendsystemproject_amd import _hip
    assert _hip.lib().rs_target_rank_splits(33, 70001, 128) > 1


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_heavy_ties(dtype):
    rng = np.random.default_rng(20)
    B, N, D = 40, 3000, 16
    Ue = rng.integers(-1, 2, (B, D)).astype(np.float32)
    Ie = rng.integers(-1, 2, (N, D)).astype(np.float32)
    Ue[3] = 0.0  # every score ties: the rank is the target's column
    tcols = _targets(rng, B, N)
    tcols[3] = 1234
    want = _check_exact(Ue, Ie, tcols, dtype)
    assert want[3] == 1234


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_history(dtype):
    rng = np.random.default_rng(7)
    B, N, D = 48, 5000, 64
    Ue = rng.integers(-3, 4, (B, D)).astype(np.float32)
    Ie = rng.integers(-3, 4, (N, D)).astype(np.float32)
    item_ids = np.arange(100, 100 + N)
    hist = _history(rng, 40, N, max_len=300)           # some users without history
    hist[7] = set(range(100, 100 + N)) - {111, 2100, 5099}   # leaves 3 columns
    hist.pop(8, None)
    users = rng.integers(0, 45, B)                      # some ids beyond the table
    users[0], users[1], users[2] = 7, 8, 44
    tcols = rng.integers(0, N, B).astype(np.int32)
    tcols[0] = 3000                                     # inside its user's history
    raw = Ue.astype(np.float64) @ Ie.astype(np.float64).T
    for b in range(8, 20):                              # a history column that outscores the target
        cols = _hist_cols(hist, users[b], N)
        if len(cols):
            best = cols[np.argmax(raw[b, cols])]
            free = np.setdiff1d(np.flatnonzero(raw[b] < raw[b, best]), cols)
            if len(free):
                tcols[b] = free[0]
    users[5] = next(u for u in range(9, 40) if len(_hist_cols(hist, u, N)))
    tcols[5] = _hist_cols(hist, users[5], N)[0]         # another masked target
    S = _mask_reference(raw, users, hist, item_ids)
    csr = sorted_history_csr(hist, item_ids, DEV)
    want = _check_exact(Ue, Ie, tcols, dtype, S=S, users=users, hist=csr)
    # a masked target: behind the 3 columns left, then the history columns below it (3000 - 2 of them)
    assert want[0] == 3 + (3000 - 2)
    outscoring = [(S[b] == -np.inf) & (raw[b] > raw[b, tcols[b]]) for b in range(B)]
    assert sum(int(o.any()) for o in outscoring) >= 8
    # no user ids: no exclusion
    _check_exact(Ue, Ie, tcols, dtype)


@pytest.mark.parametrize('with_history', [False, True])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('D', [64, 128])
def test_exact_ties_on_real_valued_data(D, dtype, with_history):
    """Copies of the target's row must tie with it bit for bit, which holds only if the target's
    score comes from the same summation order as the sweep's. Expected: the target's position in
    the list of the pre-existing fused_topk, which at K = N is the whole order."""
    g = torch.Generator().manual_seed(D + 7)
    B, N = 48, 256
    U = torch.randn(B, D, generator=g)
    items = torch.randn(N, D, generator=g)
    perm = torch.randperm(N, generator=g).tolist()
    tcols = torch.randint(0, N, (B,), generator=g).int()
    for i, b in enumerate(range(0, B, 3)):
        lo, t, hi, hi2 = sorted(perm[4 * i:4 * i + 4])  # one copy left of the target, two right of it
        items[[lo, hi, hi2]] = items[t].clone()
        tcols[b] = t
    U, items, tcols = U.to(DEV), items.to(DEV).to(DTYPES[dtype]), tcols.to(DEV)
    uids, csr = None, None
    if with_history:
        rng = np.random.default_rng(D)
        hist = {u: set(int(x) for x in rng.integers(0, N, 40)) for u in range(0, B, 2)}
        hist[0].add(int(tcols[0]))  # a duplicated target that is masked itself
        csr = sorted_history_csr(hist, np.arange(N), DEV)
        uids = torch.arange(B, device=DEV)
    order, _ = ops.fused_topk(U, items, N, uids, csr)
    want = (order == tcols.view(-1, 1)).int().argmax(dim=1).int()
    assert bool((order == tcols.view(-1, 1)).sum(dim=1).eq(1).all())
    for splits in (0, 1, 3, 8):
        got = ops.target_rank(U, items, tcols, uids, csr, splits=splits)
        assert torch.equal(got, want), (splits, (got - want).nonzero().view(-1).tolist())


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_consistent_with_topk_at_scale(dtype):
    g = torch.Generator().manual_seed(5)
    B, N, D, K = 64, 20000, 128, 50
    U = torch.randn(B, D, generator=g).to(DEV)
    items = torch.randn(N, D, generator=g).to(DEV).to(DTYPES[dtype])
    cols, _ = ops.fused_topk(U, items, K)
    # half of the targets from the user's own top list, so both outcomes occur
    tcols = torch.randint(0, N, (B,), generator=g).int().to(DEV)
    pick = torch.randint(0, K, (B,), generator=g).to(DEV)
    tcols[::2] = cols[torch.arange(0, B, 2, device=DEV), pick[::2]]
    rank = ops.target_rank(U, items, tcols)
    inside = (cols == tcols.view(-1, 1)).any(dim=1)
    assert bool(inside.any()) and not bool(inside.all())
    assert torch.equal((rank >= 0) & (rank < K), inside)
    assert torch.equal(rank[::2].long(), pick[::2])


def test_index_rank_and_columns_of():
    rng = np.random.default_rng(12)
    B, N, D = 30, 2500, 32
    Ue = rng.integers(-3, 4, (B, D)).astype(np.float32)
    Ie = rng.integers(-3, 4, (N, D)).astype(np.float32)
    item_ids = rng.permutation(np.arange(100, 100 + N))  # ids in no order: column != id - 100
    hist = _history(rng, 30, N, max_len=200)
    users = rng.integers(0, 33, B)
    tcols = rng.integers(0, N, B)
    target_ids = item_ids[tcols]
    target_ids[4] = 99  # not in the catalog
    tcols[4] = -1
    raw = Ue.astype(np.float64) @ Ie.astype(np.float64).T
    for dtype, keep in (('fp32', True), ('bf16', True), ('bf16', False)):
        index = ItemIndex.from_embeddings(_dev(Ie), _dev(item_ids), dtype=dtype, keep_fp32=keep)
        assert (index.embeddings is None) == (not keep)
        got_cols = index.columns_of(_dev(target_ids))
        assert got_cols.dtype == torch.int32 and np.array_equal(got_cols.cpu().numpy(), tcols)
        got = index.rank(_dev(Ue), _dev(target_ids))
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), np_rank(raw, tcols))
        index.set_history(hist)
        want = np_rank(_mask_reference(raw, users, hist, item_ids), tcols)
        got = index.rank(_dev(Ue), _dev(target_ids), user_ids=_dev(users))
        assert np.array_equal(got.cpu().numpy(), want) and want[4] == -1
        # rank < k exactly when search(k) returns the item
        ids, _, _ = index.search(_dev(Ue), 25, user_ids=_dev(users))
        found = (ids.cpu().numpy() == target_ids[:, None]).any(axis=1)
        assert np.array_equal(found, (want >= 0) & (want < 25))


def test_index_rank_staged_path_for_other_widths():
    rng = np.random.default_rng(14)
    B, N, D = 21, 900, 48
    Ue = rng.integers(-3, 4, (B, D)).astype(np.float32)
    Ie = rng.integers(-3, 4, (N, D)).astype(np.float32)
    item_ids = np.arange(100, 100 + N)
    hist = _history(rng, 30, N, max_len=200)
    users = rng.integers(0, 33, B)
    tcols = _targets(rng, B, N).astype(np.int64)
    target_ids = np.where((tcols >= 0) & (tcols < N), tcols + 100, 5)
    tcols[(tcols < 0) | (tcols >= N)] = -1
    some = next(b for b in range(7, B) if len(_hist_cols(hist, users[b], N)))
    tcols[some] = _hist_cols(hist, users[some], N)[0]  # a masked target
    target_ids[some] = tcols[some] + 100
    raw = Ue.astype(np.float64) @ Ie.astype(np.float64).T
    index = ItemIndex.from_embeddings(_dev(Ie), _dev(item_ids))
    got = index.rank(_dev(Ue), _dev(target_ids))
    assert np.array_equal(got.cpu().numpy(), np_rank(raw, tcols))
    index.set_history(hist)
    got = index.rank(_dev(Ue), _dev(target_ids), user_ids=_dev(users))
    assert np.array_equal(got.cpu().numpy(), np_rank(_mask_reference(raw, users, hist, item_ids), tcols))
    # more than one chunk of columns
    got = index._rank_staged(_dev(Ue), index.columns_of(_dev(target_ids)), _dev(users), index._history, chunk=256)
    assert np.array_equal(got.cpu().numpy(), np_rank(_mask_reference(raw, users, hist, item_ids), tcols))


def test_model_rank_targets():
    from recommendsystemproject_amd import synth
    cfg, m, item_loader = _demo_model()
    keys = list(m.state_dict().keys())
    index = ItemIndex.build(m, item_loader, DEV, dtype='bf16')
    batch = to_device(synth.batch_to_torch(synth.make_batch(cfg, 96, seed=31)), DEV)
    hist = {u: set(int(x) for x in np.random.default_rng(u).integers(1, len(index), 30)) for u in range(50)}
    index.set_history(hist)
    uids = _dev(np.random.default_rng(1).integers(0, 60, 96))
    targets = index.item_ids[torch.randint(0, len(index), (96,), generator=torch.Generator().manual_seed(3)).to(DEV)]
    for training in (True, False):
        m.train(training)
        got = m.rank_targets(batch['user_tower'], index, targets, user_ids=uids)
        assert m.training == training
        m.eval()
        with torch.no_grad():
            ue = m.user_tower(batch['user_tower'], m.user_feature_mapping)
        assert torch.equal(got, index.rank(ue, targets, user_ids=uids))
        assert got.shape == (96,) and got.dtype == torch.int32 and int(got.min()) >= 0
    assert list(m.state_dict().keys()) == keys


def test_evaluate_ranking_matches_validate_on_the_reference_fixture():
    """evaluate_ranking on tests/golden/validate_demo.npz, set up as
    test_validate_fused_matches_reference_fixture: its recall@k is validate(retrieval='fused')'s in
    hit counts (fp32 rows through the same tile code; unique catalog ids), and within one hit of
    the reference's recorded recall."""
    import golden_util as gu
    from recommendsystemproject_amd import synth
    from recommendsystemproject_amd.project.models.TwoTower.GenericTower import GenericTower
    from recommendsystemproject_amd.project.models.TwoTower.TwoTowerModel import TwoTowerModel
    cfg, meta, data = gu.load(os.path.join(ROOT, 'tests', 'golden', 'validate_demo.npz'))
    bn = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'validate_demo_bn.npz')))
    maps = {'user': synth.tower_layout(cfg['two_tower']['user_tower']),
            'item': synth.tower_layout(cfg['two_tower']['item_tower'])}
    m = TwoTowerModel(GenericTower(cfg, 'user_tower'), GenericTower(cfg, 'item_tower'), maps['user'], maps['item'])
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    state = synth.make_state(shapes, seed=int(meta['weight_seed']))
    state.update(bn)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    m = m.to(DEV)
    item_loader = [synth.batch_to_torch(gu.unflatten_batch(data, f'items/{j}')) for j in range(meta['item_batches'])]
    loader = [synth.batch_to_torch(gu.unflatten_batch(data, f'val/{i}')) for i in range(meta['val_batches'])]
    meta_loader = [{'user_tower': {'sparse': torch.from_numpy(data[f'uid/{i}'])}} for i in range(meta['val_batches'])]
    users, offs, items = data['hist/users'], data['hist/offs'], data['hist/items']
    hist = {int(u): set(int(x) for x in items[offs[i]:offs[i + 1]]) for i, u in enumerate(users)}
    catalog = np.concatenate([b['sparse'][:, 0].numpy() for b in item_loader])
    unique_ids = len(np.unique(catalog)) == len(catalog)
    k_list = list(meta['k_list'])
    n = sum(int(b['item_tower']['sparse'].shape[0]) for b in loader)
    m.eval()
    got = evaluate_ranking(m, loader, item_loader, DEV, k_list=[1] + k_list + [1000], meta_data_loader=meta_loader,
                           user_history=hist)
    print(got)
    assert got['num_samples'] == n and 0 < got['num_ranked'] <= n
    for k, want in zip(k_list, data['recall']):
        assert abs(got[f'recall@{k}'] - float(want)) <= 1.0 / n + 1e-12, (k, got[f'recall@{k}'], float(want))
    for k in [1] + k_list + [1000]:
        assert got[f'ndcg@{k}'] <= got[f'recall@{k}']
    assert got['recall@1'] <= got['mrr'] <= 1.0
    assert got['recall@1000'] >= got[f'recall@{max(k_list)}']
    assert 1.0 <= got['mean_rank'] <= len(catalog)
    if not unique_ids:
        pytest.skip('the fixture catalog repeats an item id: validate() counts a hit per column of the id, '
                    'so its hit counts are not comparable')
    _, acc = validate(m, loader, item_loader, DEV, epoch=None, k_list=k_list, meta_data_loader=meta_loader,
                      log_embeddings=False, user_history=hist, retrieval='fused')
    for k in k_list:
        assert round(got[f'recall@{k}'] * n) == round(acc[k] * n), (k, got[f'recall@{k}'], acc[k])
