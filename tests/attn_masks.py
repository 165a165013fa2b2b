"""Key-padding patterns that are not a prefix, for the attention tests (pure numpy: nothing here
comes from the library). One function per family: (L, seed) -> seq [B, L] int64 ids, 0 = padding.
Row 0 of every batch is a prefix sample (keys 0 .. PREFIX_LEN - 1), row 1 a full-length one, so the
known-good pattern runs in the same launch; rows COMMON .. are the family's own samples.

    all_pad   no id at all: the mask rules leave exactly key L - 1 unmasked
    lead      keys [s, L), s >= 64 when L > 64, s >= 16 when 16 < L <= 64 (s >= 1 below that)
    holes     Bernoulli(1/2) per key; key 0 padded in one sample, key L - 1 in another, both in a third
    one_mid   exactly one key, at L // 2
    tile_gap  a prefix with one whole 16-key tile zeroed in its middle (L >= 48)
    one_wave  L > 64: sample w (of 4) has keys only in the 16-key tiles tk with tk % 4 == w

seq_mask_ref is the reference's mask / last-valid rule (T6 / T7: SequenceEncoder.py:32-74) in
numpy; the cases the GPU tests run are listed here too, so that test_attn_masks_host.py can check
every (family, L) of them without a GPU."""
import numpy as np

TILE = 16    # keys per MFMA key tile
CHUNK = 64   # keys per chunk of the long forward's online softmax / per lane chunk of attn_rows
COMMON = 2   # rows 0 (prefix) and 1 (full) of every batch
PREFIX_LEN = 3
FAMILIES = ('all_pad', 'lead', 'holes', 'one_mid', 'tile_gap', 'one_wave')


def available(family, L):
    """Whether the family exists at this length."""
    return L > CHUNK if family == 'one_wave' else L >= 3 * TILE if family == 'tile_gap' else L > PREFIX_LEN


def n_tiles(L):
    return (L + TILE - 1) // TILE


def lead_min(L):
    """The smallest first valid key of a `lead` sample."""
    return CHUNK if L > CHUNK else TILE if L > TILE else 1


def _batch(family, L, seed, valid):
    """The family's valid-key rows under the two common rows, with seeded ids in [1, 1000)."""
    assert available(family, L), (family, L)
    valid = np.asarray(valid, dtype=bool).reshape(-1, L)
    common = np.zeros((COMMON, L), dtype=bool)
    common[0, :PREFIX_LEN] = True
    common[1] = True
    valid = np.concatenate([common, valid])
    rng = np.random.default_rng([seed, L, FAMILIES.index(family)])
    ids = rng.integers(1, 1000, size=valid.shape)
    return np.where(valid, ids, 0).astype(np.int64)


def all_pad(L, seed=0):
    return _batch('all_pad', L, seed, np.zeros((2, L), dtype=bool))


def lead_starts(L):
    lo = lead_min(L)
    return sorted({lo, (lo + L) // 2, L - 1})


def lead(L, seed=0):
    return _batch('lead', L, seed, [np.arange(L) >= s for s in lead_starts(L)])


def holes(L, seed=0):
    rng = np.random.default_rng([seed, L, 99])
    v = rng.random((4, L)) < 0.5
    v[0, 0], v[0, L - 1] = False, True
    v[1, 0], v[1, L - 1] = True, False
    v[2, 0] = v[2, L - 1] = False
    v[~v.any(1), L // 2] = True
    return _batch('holes', L, seed, v)


def one_mid(L, seed=0):
    v = np.zeros((2, L), dtype=bool)
    v[:, L // 2] = True
    return _batch('one_mid', L, seed, v)


def tile_gaps(L):
    """(prefix length, zeroed tile): the tile lies whole inside the prefix with valid keys on both
    sides. The second tile under a prefix one key longer than it needs (17 valid keys, the fewest
    the family allows), and under the whole length the second, a middle and the last such tile."""
    t_last = (L - 1) // TILE - 1
    return sorted({(2 * TILE + 1, 1), (L, 1), (L, (1 + t_last) // 2 + 1 if t_last > 2 else 1), (L, t_last)})


def tile_gap(L, seed=0):
    j = np.arange(L)
    return _batch('tile_gap', L, seed, [(j < n) & (j // TILE != t) for n, t in tile_gaps(L)])


def one_wave(L, seed=0):
    rng = np.random.default_rng([seed, L, 98])
    cls = (np.arange(L) // TILE) % 4
    v = np.stack([cls == w for w in range(4)])
    v[1] &= rng.random(L) < 0.5                       # a ragged subset of the class
    if not v[1].any():
        v[1, TILE] = True
    own = np.flatnonzero(v[3])
    v[3] = False
    v[3, [own[0], own[-1]]] = True                    # two keys: the class's first and last
    return _batch('one_wave', L, seed, v)


BATCH = {'all_pad': all_pad, 'lead': lead, 'holes': holes, 'one_mid': one_mid, 'tile_gap': tile_gap,
         'one_wave': one_wave}


def seq_mask_ref(seq):
    """key_pad [B, L] uint8 (1 = masked) and last [B] int64 by the reference's rules: a key is masked
    where its id is 0, except that an all-padding sample keeps key L - 1 (T6); last is the count of
    valid ids minus one, clamped at 0 -- a count, not a position (T7)."""
    seq = np.asarray(seq)
    pad = seq == 0
    pad[pad.all(1), -1] = False
    last = np.maximum((seq != 0).sum(1) - 1, 0).astype(np.int64)
    return pad.astype(np.uint8), last


def rolled(key_pad):
    """A wrong padding mask for the same batch: every sample's mask moved on by one key (the count of
    valid keys stays, so every sample keeps one)."""
    out = np.roll(np.asarray(key_pad), 1, axis=1)
    out[out.all(1), -1] = 0
    return out


# ------------------------------------------------------------------ the cases of test_gpu_attn_masks.py
# route -> (compute mode, [(L, d, H)], qkv storages (True: bf16))
ROUTES = {
    'wave_f32': ('fp32', [(L, 64, 4) for L in (7, 33, 64)], (False,)),
    'valu': ('fp32', [(50, 32, 4), (100, 64, 4)], (False,)),
    'wave_bf16': ('bf16', [(L, 64, 4) for L in (7, 33, 50, 64)], (False, True)),
    'long_bf16': ('bf16', [(L, 64, 4) for L in (65, 100, 200)], (False, True)),
}
PS = (0.0, 0.5)
ROWS_FAMILIES = ('holes', 'all_pad', 'one_mid', 'lead')
ROWS_LS = (7, 50, 100)
STEP_LS = (50, 100, 200)


def route_cases():
    """(route, mode, (L, d, H), family, stored_bf16, p): a family only at the lengths it exists at."""
    return [(route, mode, shape, fam, st, p)
            for route, (mode, shapes, storages) in ROUTES.items() for shape in shapes
            for fam in FAMILIES if available(fam, shape[0]) for st in storages for p in PS]


def family_lengths():
    """Every (family, L) a GPU test runs: the route cases, the selected-row cases, the whole steps."""
    out = {(fam, shape[0]) for _, _, shape, fam, _, _ in route_cases()}
    out |= {(fam, L) for fam in ROWS_FAMILIES for L in ROWS_LS}
    out |= {(fam, L) for L in STEP_LS for fam in FAMILIES if available(fam, L)}
    return sorted(out)


def step_valid(B, L, seed=0):
    """[B, L] bool for a whole-step batch: row b takes a sample of family b % n (the families that
    exist at L), going round the family's samples, the two common rows included."""
    fams = [f for f in FAMILIES if available(f, L)]
    pats = {f: BATCH[f](L, seed) != 0 for f in fams}
    rows = []
    for b in range(B):
        v = pats[fams[b % len(fams)]]
        rows.append(v[(COMMON + b // len(fams)) % len(v)])
    return np.stack(rows), fams
