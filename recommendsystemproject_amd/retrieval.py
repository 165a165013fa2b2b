"""Serving: top-K items for users out of a trained two-tower model.

ItemIndex holds the item tower's embeddings of a catalog (fp32, bf16 rows at half the memory, or
OCP e4m3 bytes under one power-of-two scale at a quarter: dtype='fp8') and answers `search(user_emb, k)` with the fused retrieval kernel (csrc/retrieve.hip: scores are
formed tile by tile on the MFMA and never stored). TwoTowerModel.recommend() runs the user tower
and searches an index. The result is what validate()'s staged pipeline defines (values descending,
ties by the lower catalog column, a user's history excluded).

    index = ItemIndex.build(model, item_loader, device, dtype='bf16')
    index.set_history(user_history)                       # optional: never recommend these again
    item_ids, scores, cols = model.recommend(batch['user_tower'], index, k=20, user_ids=uids)

`rank(user_emb, target_item_ids)` answers the evaluation question instead: where in that same
ordering over the WHOLE catalog does each user's held-out item stand (rs_target_rank, one integer
per user; training_utils.ranking_metrics turns it into Recall / NDCG at any k, MRR, mean rank).

    ranks = model.rank_targets(batch['user_tower'], index, target_item_ids, user_ids=uids)

Catalog filters restrict a request to a subset of the catalog inside the same two kernels (in
stock, this locale, a tombstone for a deleted item): an allow-list per filter, packed to one bit
a column on the device (rs_pack_mask), and one filter per user and request. A column outside the
user's filter scores -inf exactly as a history column does (the two combine by union), so search
still returns k items when fewer than k are allowed (the masked ones last, at -inf) and rank < k
exactly when search(k) with the same filter returns the item.

    index.set_filters({'in_stock': stock_mask, 'kids': index.mask_of(kids_item_ids)})
    item_ids, scores, cols = model.recommend(batch['user_tower'], index, k=20, filters='in_stock')
    item_ids, scores, cols = index.search(user_emb, 20, filters=per_user_filter_ids)   # < 0: none

`mine_negatives` turns the same sweep into training data: n hard negatives per user, drawn on the
device from a window of ranks of that ordering (csrc/sample.hip), never the positive, the user's
history or a column outside the user's filter; hard_negatives.NegativeMiner feeds them to a step.

    ids, cols, count = index.mine_negatives(user_emb, 10, positive_item_ids=pos, skip=0, window=31, user_ids=uids)

IvfIndex is a cluster-pruned view of an ItemIndex for catalogs where the full sweep is the cost: the
rows grouped into lists around centroids, a search sweeping only the `nprobe` lists closest to each
user (csrc/ivf.hip), defined as the exhaustive search restricted to those lists, bit for bit.

    ivf = IvfIndex.build(index, nlist=1024)
    item_ids, scores, cols = model.recommend(batch['user_tower'], ivf, k=20, user_ids=uids, nprobe=16)
"""
from __future__ import annotations

import numpy as np
import torch

from . import _hip, ops


def fused_supported(D: int) -> bool:
    """The embedding widths rs_fused_topk takes; others go through the staged retrieval_topk."""
    return 16 <= D <= 256 and D % 16 == 0


def sorted_history_csr(user_history, item_ids, device):
    """user -> catalog column indices as device CSR (off [U+1] int64, idx int32, U), with
    training_utils._history_csr's filters (ids <= the catalog's max id that are in the catalog) and
    each user's columns sorted ascending and de-duplicated: what rs_fused_topk's binary search needs."""
    ids = np.asarray(item_ids, dtype=np.int64).reshape(-1)
    max_id = int(ids.max())
    id_to_index = np.full(max_id + 1, -1, dtype=np.int64)
    id_to_index[ids] = np.arange(len(ids))

    def _uid(u):
        try:
            return int(u)
        except (TypeError, ValueError):
            return -1
    users = [_uid(u) for u in user_history.keys() if _uid(u) >= 0]
    U = (max(users) + 1) if users else 0
    counts = np.zeros(U + 1, dtype=np.int64)
    cols = []
    for u in range(U):
        items = user_history.get(u, user_history.get(np.int64(u), ()))
        valid = [int(i) for i in items if 0 <= int(i) <= max_id]
        c = id_to_index[valid] if valid else np.zeros(0, dtype=np.int64)
        c = np.unique(c[c >= 0])  # sorted, distinct
        counts[u + 1] = len(c)
        cols.append(c)
    off = np.cumsum(counts)
    idx = np.concatenate(cols).astype(np.int32) if cols and off[-1] > 0 else np.zeros(1, dtype=np.int32)
    return (torch.from_numpy(off).to(device), torch.from_numpy(idx).to(device), U)


class ItemIndex:
    """The item embeddings of a catalog, searchable by dot product. Column c of the index is row c
    of the embeddings; `item_ids[c]` is its item id."""

    def __init__(self, rows_fp32, rows_bf16, item_ids, dtype, rows_fp8=None, scale_exp=None):
        self._fp32 = rows_fp32
        self._bf16 = rows_bf16
        self._fp8 = rows_fp8        # float8_e4m3fn rows: RNE(embedding * 2^scale_exp)
        self.scale_exp = scale_exp  # None unless dtype == 'fp8'
        self.item_ids = item_ids
        self._dtype = dtype
        self._history = None
        self._by_id = None  # (sorted ids, their columns), built by the first columns_of
        self._filters = None        # packed allow-lists, uint32 [F, ceil(N / 32)] (ops.pack_mask)
        self._filter_names = None   # name -> filter id, for filters given as a dict

    @classmethod
    def from_embeddings(cls, embs, item_ids=None, dtype='fp32', keep_fp32=True):
        """dtype 'fp8': e4m3 rows under the scale ops.quantize_e4m3 picks from the largest
        magnitude (one host sync); finite embeddings of a width the fused kernels take only, as
        fp8 rows have no staged path."""
        if dtype not in ('fp32', 'bf16', 'fp8'):
            raise ValueError(f"dtype must be 'fp32', 'bf16' or 'fp8', got {dtype!r}")
        embs = embs.detach().float().contiguous()
        if dtype == 'fp8' and (embs.dim() != 2 or not fused_supported(int(embs.shape[1]))):
            raise ValueError(f'an fp8 index takes embedding widths that are a multiple of 16 in [16, 256], '
                             f'got {tuple(embs.shape)}')
        if item_ids is None:
            item_ids = torch.arange(embs.shape[0], device=embs.device, dtype=torch.int64)
        item_ids = item_ids.detach().reshape(-1).long().to(embs.device)
        if item_ids.numel() != embs.shape[0]:
            raise ValueError(f'{item_ids.numel()} item ids for {embs.shape[0]} embeddings')
        bf = embs.bfloat16() if dtype == 'bf16' else None
        q = exp = None
        if dtype == 'fp8':
            amax = float(embs.abs().max().item()) if embs.numel() else 0.0
            if not np.isfinite(amax):
                raise ValueError('an fp8 index needs finite embeddings (found inf or NaN)')
            q, exp = ops.quantize_e4m3(embs, ops.e4m3_exponent(amax))
        keep = dtype == 'fp32' or keep_fp32
        return cls(embs if keep else None, bf, item_ids, dtype, q, exp)

    @classmethod
    def build(cls, model, item_loader, device, dtype='fp32', item_id_feature='movie_id_enc',
              item_id_type='sparse', item_id_col=0, keep_fp32=True):
        """validate()'s indexing loop: the item tower in eval mode over the loader's batches."""
        from .project.utils.training_utils import extract_item_id, to_device
        was_training = model.training
        model.eval()
        embs, ids = [], []
        try:
            with torch.no_grad():
                for item_batch in item_loader:
                    item_batch = to_device(item_batch, device)
                    embs.append(model.get_item_embeddings(item_batch))
                    ids.append(extract_item_id(item_batch, feature_name=item_id_feature, feature_type=item_id_type,
                                               item_id_col=item_id_col))
        finally:
            model.train(was_training)
        return cls.from_embeddings(torch.cat(embs, dim=0), torch.cat(ids, dim=0).view(-1).long(), dtype=dtype,
                                   keep_fp32=keep_fp32)

    def __len__(self):
        return int(self.item_ids.numel())

    @property
    def dim(self):
        return int(self._rows().shape[1])

    @property
    def dtype(self):
        return self._dtype

    @property
    def embeddings(self):
        """The fp32 rows (None for a bf16 or fp8 index built with keep_fp32=False)."""
        return self._fp32

    def _rows(self):
        return {'bf16': self._bf16, 'fp8': self._fp8}.get(self._dtype, self._fp32)

    def set_history(self, user_history):
        """Exclude each user's items (user -> iterable of item ids, as build_user_history makes)
        from that user's results; None clears it. search() then needs user_ids."""
        self._history = None
        if user_history is not None:
            self._history = sorted_history_csr(user_history, self.item_ids.cpu().numpy(), self.item_ids.device)

    def set_filters(self, masks):
        """Catalog filters: each an allow-list over the catalog's columns, in column order. masks:
        a bool / uint8 tensor or array [F, N] or [N] (nonzero = allowed; filter ids 0 .. F - 1),
        or a dict name -> [N] mask (ids in the dict's order, names usable in search / rank); None
        clears them. Only the packed words stay, on the index's device (N / 8 bytes a filter;
        packed there by rs_pack_mask, or on the host for an index that lives on the host, which
        cannot search).
        search / rank then take filters=. A filter is applied inside the fused kernels, which still
        sweep the whole catalog: for a filter that keeps a very small part of it, a compact
        sub-index (from_embeddings on the allowed rows) reads far less. To combine filters, AND
        their masks here."""
        if masks is None:
            self._filters = self._filter_names = None
            return
        names = None
        if isinstance(masks, dict):
            if not masks:
                raise ValueError('set_filters: an empty dict of filters (None clears them)')
            names = {name: i for i, name in enumerate(masks)}
            rows = [torch.as_tensor(np.asarray(m) if not torch.is_tensor(m) else m).reshape(-1) for m in masks.values()]
            for name, r in zip(masks, rows):
                if r.numel() != len(self):
                    raise ValueError(f'set_filters: filter {name!r} has {r.numel()} columns, the catalog {len(self)}')
            m = torch.stack([r.to(self.item_ids.device) != 0 for r in rows])
        else:
            m = torch.as_tensor(np.asarray(masks) if not torch.is_tensor(masks) else masks)
            if m.dim() == 1:
                m = m.view(1, -1)
            if m.dim() != 2 or m.shape[0] < 1 or m.shape[1] != len(self):
                raise ValueError(f'set_filters: masks [F, N] or [N] with N = {len(self)} catalog columns, '
                                 f'got {tuple(m.shape)}')
            if m.dtype not in (torch.bool, torch.uint8):
                raise ValueError(f'set_filters: bool or uint8 masks, got {m.dtype}')
            m = m.to(self.item_ids.device)
        if m.is_cuda:
            self._filters = ops.pack_mask(m)
        else:  # a host index: the same words (little-endian bit order), no device to pack on
            b = np.packbits(m.numpy() != 0, axis=1, bitorder='little')
            b = np.pad(b, ((0, 0), (0, -b.shape[1] % 4)))
            self._filters = torch.from_numpy(np.ascontiguousarray(b).view('<u4').astype(np.int64)).to(torch.uint32)
        self._filter_names = names

    @property
    def num_filters(self):
        return 0 if self._filters is None else int(self._filters.shape[0])

    def mask_of(self, item_ids):
        """bool [N] on the index's device: True at every catalog column whose item id is listed
        (every column of an id the catalog holds twice; an id it does not hold marks nothing), so
        an allow-list of ids becomes a filter: set_filters(index.mask_of(ids))."""
        q = torch.as_tensor(item_ids).reshape(-1).long().to(self.item_ids.device)
        return torch.isin(self.item_ids, q)

    def _filter_ids(self, filters, B, device):
        """search / rank's `filters` -> int32 [B] on the device (negative: unfiltered), or None."""
        if filters is None:
            return None
        if self._filters is None:
            raise ValueError('filters given, but the index has none: call set_filters first')
        if not fused_supported(self.dim):
            raise ValueError(f'catalog filters run in the fused kernels only: embedding widths that are a multiple '
                             f'of 16 in [16, 256], got {self.dim}')
        if torch.is_tensor(filters) or isinstance(filters, (np.ndarray, list, tuple)):
            f = torch.as_tensor(filters)
            if f.is_floating_point() or f.dtype == torch.bool or f.numel() != B:
                raise ValueError(f'filters: an int, a name or an integer tensor [B = {B}], got {f.dtype} '
                                 f'{tuple(f.shape)}')
            return f.reshape(-1).to(device)
        if not isinstance(filters, (int, np.integer)) or isinstance(filters, bool):  # a name
            if self._filter_names is None or filters not in self._filter_names:
                raise ValueError(f'unknown filter {filters!r}: the index has '
                                 f'{list(self._filter_names) if self._filter_names else self.num_filters}')
            filters = self._filter_names[filters]
        if not 0 <= int(filters) < self.num_filters:
            raise ValueError(f'filter {int(filters)} out of range: the index has {self.num_filters}')
        return torch.full((B,), int(filters), device=device, dtype=torch.int32)

    def search(self, user_emb, k, user_ids=None, oversample=1, filters=None):
        """-> (item_ids int64 [B, k], scores fp32 [B, k], cols int32 [B, k]), best first.
        filters: one of set_filters' filters for every user (its int id or its name), or an integer
        tensor [B] of ids, negative = that user unfiltered. Columns outside the filter come last,
        at -inf, and only when fewer than k are allowed."""
        rows = self._rows()
        k = int(k)
        if k < 1 or k > len(self):
            raise ValueError(f'selected index k out of range (k={k}, items={len(self)})')
        if oversample > 1 and self._fp32 is None:
            raise ValueError('oversample > 1 rescores with the fp32 rows: build the index with keep_fp32=True')
        fid = self._filter_ids(filters, int(user_emb.shape[0]), rows.device)
        _hip.require_device(user_emb)
        _hip.require_device(rows)
        hist = self._history if user_ids is not None else None
        U = user_emb.detach().float().contiguous()
        flt = dict(filter_ids=fid, filters=self._filters) if fid is not None else {}
        if not fused_supported(self.dim):
            cols, val = self._search_staged(U, k, user_ids, hist)
        elif oversample > 1 and self._dtype != 'fp32':
            C = min(256, int(oversample) * k, len(self))
            cand, cval = ops.fused_topk(U, rows, C, user_ids, hist, item_exp=self.scale_exp, **flt)
            exact = ops.rescore_rows(U, self._fp32, cand, cval)
            cols = torch.empty(U.shape[0], k, device=U.device, dtype=torch.int32)
            val = torch.empty(U.shape[0], k, device=U.device, dtype=torch.float32)
            _hip.call('rs_topk_rows', exact.data_ptr(), C, int(U.shape[0]), C, k, cand.data_ptr(), C, 0,
                      cols.data_ptr(), val.data_ptr(), k, ops.stream())
        else:
            cols, val = ops.fused_topk(U, rows, k, user_ids, hist, item_exp=self.scale_exp, **flt)
        return self.item_ids[cols.long()], val, cols

    def mine_negatives(self, user_emb, n, positive_item_ids=None, skip=0, window=None, user_ids=None, filters=None,
                       seed=0, draw=0):
        """Hard negatives from the model's own ordering, chosen on the device: for each user, n
        items drawn uniformly without replacement from the ranks [skip, skip + window) of search's
        order, counted over the ELIGIBLE items only: not in the user's history (user_ids, as
        search), inside the user's filter (filters, as search), and not the user's positive
        (positive_item_ids [B]: the test is on the item id, so every column holding that id is
        excluded). -> (ids int64 [B, n], cols int32 [B, n], count int32 [B]), ready for
        ItemCatalog.materialize(ids).

        window=None means min(255 - skip, N). skip leaves out the very top, where unlabelled
        positives sit. When fewer than skip + window eligible items exist, the window slides
        towards the top only as far as needed to hold n. count[b] = n normally; a pool of
        0 < P < n members is returned whole, in drawn order, repeated cyclically, with
        count[b] = P; an empty pool gives ids and cols -1 and count[b] = 0 (materialize flags
        such ids), so read count where the filters can be that tight. The draw is a pure function
        of (seed, draw, user row, column): the same arguments give the same tensors, on every
        index dtype with the same ordering; advance `draw` per call for fresh samples.

        The sweep fetches C = min(skip + window + 1, N) candidates, the + 1 covering the
        positive's own column. A catalog that holds the positive's id in several columns can leave
        the pool that many entries short at its tail; count reports it and nothing compensates.
        C <= 32 runs the sweep's four-wave small-K kernel, C up to 256 the one-wave one: a shallow
        window (skip + window <= 31) is the cheap setting for mining every step. Embedding widths
        outside fused_supported have no staged path here."""
        rows = self._rows()
        N = len(self)
        n, skip = int(n), int(skip)
        if not fused_supported(self.dim):
            raise ValueError(f'mine_negatives runs on the fused sweep only: embedding widths that are a multiple '
                             f'of 16 in [16, 256], got {self.dim}')
        if skip < 0:
            raise ValueError(f'mine_negatives: skip = {skip} < 0')
        window = min(255 - skip, N) if window is None else int(window)
        if skip + window > 255:
            raise ValueError(f'mine_negatives: skip + window = {skip + window} > 255, the deepest window the sweep '
                             f'fetches')
        if n < 1 or n > window:
            raise ValueError(f'mine_negatives: n = {n} outside [1, window = {window}]')
        B = int(user_emb.shape[0])
        pos = None
        if positive_item_ids is not None:
            pos = torch.as_tensor(positive_item_ids).reshape(-1)
            if pos.numel() != B:
                raise ValueError(f'mine_negatives: {pos.numel()} positive items for {B} users')
            pos = pos.to(rows.device)
        fid = self._filter_ids(filters, B, rows.device)
        _hip.require_device(user_emb)
        _hip.require_device(rows)
        hist = self._history if user_ids is not None else None
        U = user_emb.detach().float().contiguous()
        flt = dict(filter_ids=fid, filters=self._filters) if fid is not None else {}
        C = min(skip + window + 1, N)
        cand, cval = ops.fused_topk(U, rows, C, user_ids, hist, item_exp=self.scale_exp, **flt)
        return ops.sample_negatives(cand, cval, self.item_ids, pos, skip, window, n, seed=seed, draw=draw)

    def columns_of(self, item_ids):
        """item ids -> their catalog columns, int32 of the same shape on the index's device; -1 for
        an id that is not in the catalog. An id the catalog holds twice maps to its last column
        (the reference's id_to_index_map assignment keeps the last writer)."""
        if self._by_id is None:  # built once: the ids sorted (stable, so equal ids keep column order)
            sorted_ids, order = torch.sort(self.item_ids, stable=True)
            self._by_id = (sorted_ids.contiguous(), order.int())
        sorted_ids, order = self._by_id
        q = torch.as_tensor(item_ids).to(sorted_ids.device).long()
        flat = q.reshape(-1).contiguous()
        if sorted_ids.numel() == 0:
            return torch.full_like(q, -1, dtype=torch.int32)
        pos = (torch.searchsorted(sorted_ids, flat, right=True) - 1).clamp(min=0)  # the last equal id
        cols = torch.where(sorted_ids[pos] == flat, order[pos], torch.full_like(order[pos], -1))
        return cols.reshape(q.shape)

    def rank(self, user_emb, target_item_ids, user_ids=None, filters=None):
        """-> int32 [B]: the 0-based position of each user's target item in the full ordering that
        search() takes its first k from (value descending, ties by the lower column, the user's
        history at -inf, the target's own membership included), so rank < k exactly when search(k)
        returns the item; -1 for an item id the catalog does not hold. One pass of the fused rank
        kernel (ops.target_rank) on the index's own rows, any catalog size, no score matrix: there
        a column holding a copy of the target's row ties with it bit for bit. Embedding widths the
        kernel does not take (fused_supported) go through the staged pieces chunk by chunk against
        the gathered target score: the same definition, but the target's score is summed in another
        order than the chunk's, so equal rows need not tie exactly. filters as search's: a target
        outside the user's filter ranks behind every allowed column."""
        rows = self._rows()
        fid = self._filter_ids(filters, int(user_emb.shape[0]), rows.device)
        _hip.require_device(user_emb)
        _hip.require_device(rows)
        hist = self._history if user_ids is not None else None
        U = user_emb.detach().float().contiguous()
        cols = self.columns_of(torch.as_tensor(target_item_ids).reshape(-1))
        if cols.numel() != U.shape[0]:
            raise ValueError(f'{cols.numel()} target items for {U.shape[0]} users')
        if fused_supported(self.dim):
            flt = dict(filter_ids=fid, filters=self._filters) if fid is not None else {}
            return ops.target_rank(U, rows, cols, user_ids, hist, item_exp=self.scale_exp, **flt)
        return self._rank_staged(U, cols, user_ids, hist)

    def _rank_staged(self, U, cols, user_ids, hist, chunk=65536):
        """Embedding widths the fused kernel does not take: per column chunk the GEMM scores and
        the device history mask, compared against the gathered (and equally masked) target score."""
        rows = self._fp32 if self._fp32 is not None else self._bf16.float()
        B, D = int(U.shape[0]), int(U.shape[1])
        N = len(self)
        tcol = cols.long().view(-1, 1)
        gather = cols.clamp(min=0).view(-1, 1).contiguous()
        ts = ops.rescore_rows(U, rows, gather)
        uid = None
        if hist is not None:
            uid = user_ids.long().reshape(-1).contiguous()
            _hip.require_device(uid)
            ts = self._mask_gathered(ts, gather, uid, hist, N)
        count = torch.zeros(B, device=U.device, dtype=torch.int64)
        S = torch.empty(B * min(chunk, N), device=U.device, dtype=torch.float32)
        for c0 in range(0, N, chunk):
            n = min(chunk, N - c0)
            Sc = S[:B * n].view(B, n)
            ops.gemm(U, rows[c0:c0 + n], Sc, B, n, D, transA=0, transB=1, lda=D, ldb=D, ldc=n)
            if hist is not None:
                off, idx, nu = hist
                _hip.call('rs_mask_history', Sc.data_ptr(), n, B, c0, n, uid.data_ptr(), int(uid.stride(0)),
                          off.data_ptr(), idx.data_ptr(), nu, ops.stream())
            col = torch.arange(c0, c0 + n, device=U.device).view(1, -1)
            ahead = (Sc > ts) | ((Sc == ts) & (col < tcol))
            count += (ahead & (col != tcol)).sum(dim=1)
        return torch.where(tcol.view(-1) >= 0, count, torch.full_like(count, -1)).int()

    def _search_staged(self, U, k, user_ids, hist):
        """Embedding widths the fused kernel does not take: the staged pipeline, scores gathered."""
        from .project.utils.training_utils import retrieval_topk
        rows = self._fp32 if self._fp32 is not None else self._bf16.float()
        uid = user_ids.long() if user_ids is not None else None
        cols = retrieval_topk(U, rows, k, uid, hist)
        val = ops.rescore_rows(U, rows, cols)
        if hist is not None:
            val = self._mask_gathered(val, cols, uid.reshape(-1), hist, len(self))
        return cols, val

    @staticmethod
    def _mask_gathered(val, cols, uid, hist, ncols):
        """-inf at the gathered scores whose column is in the user's history slice: the CSR is
        user-major and sorted within a user, so user * ncols + column is one sorted key array."""
        off, idx, nu = hist
        total = int(off[-1].item()) if nu else 0
        if total == 0:
            return val
        owner = torch.repeat_interleave(torch.arange(nu, device=off.device), off[1:] - off[:-1])
        keys = owner * ncols + idx[:total].long()
        ok = (uid >= 0) & (uid < nu)
        q = uid.clamp(0, nu - 1).view(-1, 1) * ncols + cols.long()
        pos = torch.searchsorted(keys, q.contiguous()).clamp(max=total - 1)
        hit = (keys[pos] == q) & ok.view(-1, 1)
        return val.masked_fill(hit, float('-inf'))


class IvfIndex:
    """A cluster-pruned (IVF) view of an ItemIndex: the catalog's rows grouped into `nlist` lists
    around centroids on the sphere; a search scores the user against the centroids and sweeps only
    the `nprobe` closest lists (csrc/ivf.hip) instead of the whole catalog.

    The result is DEFINED as the base index's exhaustive search restricted to the probed lists:
    masked score descending, ties by the lower catalog column, the user's history and the columns
    outside the user's filter excluded, over the columns c with assign[c] in the user's probed
    lists. Scores have the bits the exhaustive sweep gives the same (user, column), so with
    nprobe == nlist the two searches agree exactly. Only entries above -inf are returned: when the
    probed lists hold fewer than k eligible columns the rest is (item id -1, score -inf, column -1);
    unlike ItemIndex.search a masked column never comes back.

    The base index stays as `base`: history (set_history), filters (set_filters), item_ids,
    columns_of, mask_of, rank and mine_negatives are the base's, stay exhaustive, and what is set
    there applies to search here. Columns are the catalog's throughout; the cluster-sorted order is
    internal.

    Cost beside the base: one more copy of the rows (in the base's dtype), 4 N bytes of `perm` and
    nlist * D * 4 bytes of centroids.

        ivf = IvfIndex.build(index, nlist=1024)
        item_ids, scores, cols = ivf.search(user_emb, 20, nprobe=16, user_ids=uids)
    """

    def __init__(self, base, centroids, rows_sorted, perm, list_off, assign):
        self.base = base
        self.centroids = centroids      # fp32 [nlist, D]
        self.rows_sorted = rows_sorted  # the base's rows, grouped by list
        self.perm = perm                # int32 [N]: the catalog column of sorted row r
        self.list_off = list_off        # int32 [nlist + 1]
        self.assign = assign            # int32 [N]: the list of catalog column c

    @property
    def nlist(self):
        return int(self.centroids.shape[0])

    def __len__(self):
        return len(self.base)

    @classmethod
    def from_assignment(cls, index, centroids, assign):
        """The index for a given clustering: centroids fp32 [nlist, D], assign integer [N] with
        values in [0, nlist) (a list may be empty). The sort by list is stable, so the rows of one
        list stay in ascending catalog column. Runs on the base's device, host tensors included."""
        rows = index._rows()
        N, D = int(rows.shape[0]), int(rows.shape[1])
        dev = rows.device
        centroids = torch.as_tensor(centroids).detach().float().to(dev).contiguous()
        if centroids.dim() != 2 or int(centroids.shape[1]) != D or centroids.shape[0] < 1:
            raise ValueError(f'from_assignment: centroids [nlist >= 1, D = {D}], got {tuple(centroids.shape)}')
        nlist = int(centroids.shape[0])
        if nlist > 65536:
            raise ValueError(f'from_assignment: nlist = {nlist}, at most 65536')
        if not fused_supported(D):
            raise ValueError(f'an IvfIndex takes embedding widths that are a multiple of 16 in [16, 256], got {D}')
        a = torch.as_tensor(assign).detach().reshape(-1)
        if a.is_floating_point() or a.dtype == torch.bool or a.numel() != N:
            raise ValueError(f'from_assignment: assign integer [N = {N}], got {a.dtype} {tuple(a.shape)}')
        a = a.to(dev).long()
        if N and (int(a.min()) < 0 or int(a.max()) >= nlist):
            raise ValueError(f'from_assignment: assign values outside [0, nlist = {nlist})')
        order = torch.sort(a, stable=True).indices
        counts = torch.bincount(a, minlength=nlist)
        list_off = torch.zeros(nlist + 1, device=dev, dtype=torch.int64)
        list_off[1:] = torch.cumsum(counts, 0)
        # float8 rows move as bytes (no gather kernel for the dtype)
        src = rows.view(torch.uint8) if rows.dtype == torch.float8_e4m3fn else rows
        rows_sorted = src.index_select(0, order).contiguous()
        if rows.dtype == torch.float8_e4m3fn:
            rows_sorted = rows_sorted.view(torch.float8_e4m3fn)
        return cls(index, centroids, rows_sorted, order.int().contiguous(), list_off.int().contiguous(),
                   a.int().contiguous())

    @classmethod
    def build(cls, index, nlist, iters=10, seed=0):
        """Spherical k-means on the base's fp32 rows: `nlist` distinct rows drawn by a seeded CPU
        generator as the first centroids, then `iters` rounds of assignment (ops.fused_topk of the
        rows against the centroids, K = 1: ties to the lower list) and update (the normalised mean
        of a list's members, summed in column order; an emptied list keeps its centroid). The same
        seed gives the same index, bit for bit. Off the serving path: it synchronises freely."""
        X = index.embeddings
        if X is None:
            raise ValueError('IvfIndex.build clusters the fp32 rows: build the base index with keep_fp32=True')
        N, D = int(X.shape[0]), int(X.shape[1])
        nlist, iters = int(nlist), int(iters)
        if not 1 <= nlist <= min(N, 65536):
            raise ValueError(f'IvfIndex.build: nlist = {nlist}, must be in [1, min(N = {N}, 65536)]')
        if iters < 0:
            raise ValueError(f'IvfIndex.build: iters = {iters} < 0')
        if not fused_supported(D):
            raise ValueError(f'an IvfIndex takes embedding widths that are a multiple of 16 in [16, 256], got {D}')
        _hip.require_device(X)
        g = torch.Generator(device='cpu')
        g.manual_seed(int(seed))
        first = torch.randperm(N, generator=g)[:nlist].to(X.device)
        C = torch.nn.functional.normalize(X.index_select(0, first), dim=1).contiguous()
        for _ in range(iters):
            a = ops.fused_topk(X, C, 1)[0].view(-1).long()
            # member sums in column order (a stable sort, then one sequential sum per list and
            # dimension): index_add_'s atomics would make the centroids' last bits vary by run
            order = torch.sort(a, stable=True).indices
            sums = torch.segment_reduce(X.index_select(0, order), 'sum', lengths=torch.bincount(a, minlength=nlist),
                                        axis=0, unsafe=True)
            norm = sums.norm(dim=1, keepdim=True)
            C = torch.where(norm > 0, sums / norm.clamp(min=1e-30), C).contiguous()
        assign = ops.fused_topk(X, C, 1)[0].view(-1)
        return cls.from_assignment(index, C, assign)

    def search(self, user_emb, k, nprobe, user_ids=None, filters=None):
        """-> (item_ids int64 [B, k], scores fp32 [B, k], cols int32 [B, k]), best first, from the
        nprobe lists closest to each user; (-1, -inf, -1) where the probed lists hold fewer than k
        eligible columns. user_ids and filters as ItemIndex.search's (the base's history and
        filters). Nothing here synchronises with the host."""
        base = self.base
        k, nprobe = int(k), int(nprobe)
        if k < 1 or k > 256:
            raise ValueError(f'IvfIndex.search: k = {k}, must be in [1, 256]')
        if not 1 <= nprobe <= min(self.nlist, 256):
            raise ValueError(f'IvfIndex.search: nprobe = {nprobe}, must be in [1, min(nlist = {self.nlist}, 256)]')
        fid = base._filter_ids(filters, int(user_emb.shape[0]), self.rows_sorted.device)
        _hip.require_device(user_emb)
        _hip.require_device(self.rows_sorted)
        hist = base._history if user_ids is not None else None
        U = user_emb.detach().float().contiguous()
        flt = dict(filter_ids=fid, filters=base._filters) if fid is not None else {}
        cols, val = ops.ivf_topk(U, self.rows_sorted, self.perm, self.list_off, self.centroids, k, nprobe, user_ids,
                                 hist, item_exp=base.scale_exp, **flt)
        ids = torch.where(cols >= 0, base.item_ids[cols.clamp(min=0).long()], torch.full_like(cols, -1, dtype=torch.int64))
        return ids, val, cols
