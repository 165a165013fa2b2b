"""The mask families of tests/attn_masks.py have the properties the GPU tests count on, at every
(family, L) those tests run: checked here in numpy, so a GPU test can never quietly run on a mask
that misses the branch it is there for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_masks as am  # noqa: E402

CASES = am.family_lengths()


def _masks(family, L):
    seq = am.BATCH[family](L)
    key_pad, last = am.seq_mask_ref(seq)
    return seq, ~key_pad.astype(bool), last


def test_every_route_length_has_every_family_it_can():
    got = {}
    for fam, L in CASES:
        got.setdefault(L, set()).add(fam)
    for L, fams in got.items():
        want = {f for f in am.FAMILIES if am.available(f, L)}
        assert fams == want, (L, fams)
    assert {f for f, L in CASES if L == 200} == set(am.FAMILIES)
    assert not am.available('tile_gap', 33) and not am.available('one_wave', 64)
    ids = [(r, s, f, st, p) for r, _, s, f, st, p in am.route_cases()]
    assert len(set(ids)) == len(ids)


def test_mask_rules_on_the_pinned_quirks():
    # test_seq_mask_quirks' rows
    key_pad, last = am.seq_mask_ref(np.array([[5, 3, 0, 0], [0, 0, 0, 0], [1, 2, 3, 4], [0, 7, 0, 0]]))
    assert key_pad.tolist() == [[0, 0, 1, 1], [1, 1, 1, 0], [0, 0, 0, 0], [1, 0, 1, 1]]
    assert last.tolist() == [1, 0, 3, 0]


@pytest.mark.parametrize('family,L', CASES, ids=[f'{f}-L{L}' for f, L in CASES])
def test_family_has_its_property(family, L):
    seq, valid, last = _masks(family, L)
    B = seq.shape[0]
    assert seq.shape == (B, L) and seq.dtype == np.int64 and am.COMMON < B <= 8
    assert valid.any(1).all()  # after the all-padding rewrite every sample has a key
    # the two common rows: a prefix (shorter than L) and a full sample
    assert valid[0].tolist() == (np.arange(L) < am.PREFIX_LEN).tolist() and am.PREFIX_LEN < L
    assert valid[1].all()
    own, ids = valid[am.COMMON:], seq[am.COMMON:]
    prefix = np.array([v[:v.sum()].all() for v in own])
    assert not prefix.any()  # no sample of a family is a prefix mask
    tile_any = np.stack([np.pad(v, (0, am.n_tiles(L) * am.TILE - L)).reshape(-1, am.TILE).any(1) for v in own])
    if family == 'all_pad':
        assert not ids.any()
        assert (own.sum(1) == 1).all() and own[:, L - 1].all()
    if family in ('all_pad', 'lead'):
        # chunk 0 (L > 64) / the first key tile (16 < L <= 64) / key 0 has no valid key
        assert not own[:, :am.lead_min(L)].any()
    if family == 'lead':
        assert [int(v.argmax()) for v in own] == am.lead_starts(L)
        assert all(v[s:].all() for v, s in zip(own, am.lead_starts(L)))
        assert min(am.lead_starts(L)) == am.lead_min(L) and max(am.lead_starts(L)) == L - 1
    if family == 'holes':
        assert (~own[:, 0]).any() and (~own[:, L - 1]).any()  # leading and trailing padding
        assert own[~own[:, 0], L - 1].any() and own[~own[:, L - 1], 0].any()  # and each on its own
        # valid keys in more than one run: the ballot bits are not contiguous
        runs = (np.diff(np.pad(own, ((0, 0), (1, 1))).astype(np.int8), axis=1) == 1).sum(1)
        assert (runs > 1).sum() >= 3 and ((runs > 1).all() or L < 16)
        frac = own.mean()
        assert 0.3 < frac < 0.7 or L < 16
    if family == 'one_mid':
        assert (own.sum(1) == 1).all() and own[:, L // 2].all() and 0 < L // 2 < L - 1
    if family == 'tile_gap':
        for v, t, (n, gap) in zip(own, tile_any, am.tile_gaps(L)):
            assert not t[gap] and t[:gap].all() and t[gap + 1:am.n_tiles(n)].all() and gap + 1 < am.n_tiles(n)
            assert v.sum() == n - am.TILE and not v[n:].any()
        assert min(v.sum() for v in own) == am.TILE + 1
    if family == 'one_wave':
        assert len(own) == 4 and L > am.CHUNK
        for w, t in enumerate(tile_any):  # NT = ceil(L / 16) tiles: none of another residue class
            assert t.any() and all(tk % 4 == w for tk in np.flatnonzero(t)), (w, t)
        # the shared-tile merge meets a wave with no key as wave 0, 1, 2 and 3
        assert all(any(not t[w::4].any() for t in tile_any) for w in range(4))


@pytest.mark.parametrize('family,L', CASES, ids=[f'{f}-L{L}' for f, L in CASES])
def test_rolled_mask_is_another_legal_mask(family, L):
    _, valid, _ = _masks(family, L)
    wrong = ~am.rolled(~valid).astype(bool)
    assert wrong.any(1).all() and (wrong.sum(1) == valid.sum(1)).all()
    assert (wrong != valid).any(1).sum() >= valid.shape[0] - 1  # every sample but the full one


@pytest.mark.parametrize('L', am.ROWS_LS)
@pytest.mark.parametrize('family', am.ROWS_FAMILIES)
def test_selected_row_sits_on_padding(family, L):
    """last[b] counts the valid ids, so under interior or leading padding the selected query row is a
    padded position ([0, 7, 0, 0] -> last 0 of test_seq_mask_quirks, scaled up)."""
    _, valid, last = _masks(family, L)
    on_pad = ~valid[np.arange(len(last)), last]
    assert on_pad[am.COMMON:].any(), (family, L, last)
    assert not on_pad[:am.COMMON].any()


@pytest.mark.parametrize('L', am.STEP_LS)
def test_step_rows_hold_every_family(L):
    B = {50: 48, 100: 24, 200: 164}[L]
    valid, fams = am.step_valid(B, L)
    assert valid.shape == (B, L) and fams == [f for f in am.FAMILIES if am.available(f, L)]
    for k, f in enumerate(fams):
        pats = am.BATCH[f](L) != 0
        rows = valid[k::len(fams)]
        assert all(any((r == q).all() for q in pats) for r in rows)
        assert any((r == pats[am.COMMON]).all() for r in rows)
    key_pad, last = am.seq_mask_ref(valid.astype(np.int64))
    assert (key_pad[np.arange(B), last] == 1).any() and (~valid.any(1)).any()
