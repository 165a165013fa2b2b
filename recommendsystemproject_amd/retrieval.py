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

    def search(self, user_emb, k, user_ids=None, oversample=1):
        """-> (item_ids int64 [B, k], scores fp32 [B, k], cols int32 [B, k]), best first."""
        rows = self._rows()
        k = int(k)
        if k < 1 or k > len(self):
            raise ValueError(f'selected index k out of range (k={k}, items={len(self)})')
        if oversample > 1 and self._fp32 is None:
            raise ValueError('oversample > 1 rescores with the fp32 rows: build the index with keep_fp32=True')
        _hip.require_device(user_emb)
        _hip.require_device(rows)
        hist = self._history if user_ids is not None else None
        U = user_emb.detach().float().contiguous()
        if not fused_supported(self.dim):
            cols, val = self._search_staged(U, k, user_ids, hist)
        elif oversample > 1 and self._dtype != 'fp32':
            C = min(256, int(oversample) * k, len(self))
            cand, cval = ops.fused_topk(U, rows, C, user_ids, hist, item_exp=self.scale_exp)
            exact = ops.rescore_rows(U, self._fp32, cand, cval)
            cols = torch.empty(U.shape[0], k, device=U.device, dtype=torch.int32)
            val = torch.empty(U.shape[0], k, device=U.device, dtype=torch.float32)
            _hip.call('rs_topk_rows', exact.data_ptr(), C, int(U.shape[0]), C, k, cand.data_ptr(), C, 0,
                      cols.data_ptr(), val.data_ptr(), k, ops.stream())
        else:
            cols, val = ops.fused_topk(U, rows, k, user_ids, hist, item_exp=self.scale_exp)
        return self.item_ids[cols.long()], val, cols

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

    def rank(self, user_emb, target_item_ids, user_ids=None):
        """-> int32 [B]: the 0-based position of each user's target item in the full ordering that
        search() takes its first k from (value descending, ties by the lower column, the user's
        history at -inf, the target's own membership included), so rank < k exactly when search(k)
        returns the item; -1 for an item id the catalog does not hold. One pass of the fused rank
        kernel (ops.target_rank) on the index's own rows, any catalog size, no score matrix: there
        a column holding a copy of the target's row ties with it bit for bit. Embedding widths the
        kernel does not take (fused_supported) go through the staged pieces chunk by chunk against
        the gathered target score: the same definition, but the target's score is summed in another
        order than the chunk's, so equal rows need not tie exactly."""
        rows = self._rows()
        _hip.require_device(user_emb)
        _hip.require_device(rows)
        hist = self._history if user_ids is not None else None
        U = user_emb.detach().float().contiguous()
        cols = self.columns_of(torch.as_tensor(target_item_ids).reshape(-1))
        if cols.numel() != U.shape[0]:
            raise ValueError(f'{cols.numel()} target items for {U.shape[0]} users')
        if fused_supported(self.dim):
            return ops.target_rank(U, rows, cols, user_ids, hist, item_exp=self.scale_exp)
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
