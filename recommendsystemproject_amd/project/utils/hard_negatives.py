"""Hard-negative materialisation on the device.

The reference prepares hard-negative item ids in preprocessing (parsing.py:215-250:
`hard_neg_ids`, N same-genre unseen movies per positive) and the model consumes
`batch['hard_negatives']` = a list of N item-tower dicts (TwoTowerModel.py:53-60), but its
loader leaves building that list as a TODO (CombineTwoTower.py:86-90). Here an `ItemCatalog`
keeps every item's item-tower features on the device and materialises the N dicts for a batch
of ids with one gather kernel per feature block (rs_catalog_gather). The N slots are written
stacked as one [N*B] batch; the list holds views of it, and `TwoTowerModel.forward` runs the
item tower ONCE over the stack with per-slot BatchNorm statistics (identical to the N separate
passes of the reference, T13).

    catalog = ItemCatalog(sparse=item_sparse, sequence={'genre_ids': item_genres})
    batch['hard_negatives'] = catalog.materialize(neg_ids)      # neg_ids [B, N] int64, device

The ids can come from preprocessing, as in the reference, or from the model being trained:
`NegativeMiner` draws them on the device from a window of ranks of the model's own ordering over a
retrieval.ItemIndex (csrc/sample.hip) and attaches them to each batch (train_step(miner=)).
"""
from __future__ import annotations

import numpy as np
import torch

from recommendsystemproject_amd import _hip


class HardNegativeList(list):
    """The N item-tower dicts (views into `stacked`, the [N*B] batch they were written into)."""

    stacked = None


def _to_device(a, dev, as_float=False):
    t = torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a)
    if t.dim() == 1:
        t = t.unsqueeze(1)
    if as_float:
        t = t.to(torch.float32)
    elif t.dtype not in (torch.int32, torch.int64):
        t = t.to(torch.int64)
    elif t.dtype == torch.int64 and int(t.max()) < 2 ** 31 and int(t.min()) >= -2 ** 31:
        t = t.to(torch.int32)  # half the catalog bytes; widened to int64 by the gather
    return t.contiguous().to(dev)


class ItemCatalog:
    """Item-tower features of every item, indexed by item id (row = id).

    sparse   [V, S] integer: the item tower's `sparse` columns (config order / mapping order)
    sequence {name: [V, T]} integer: pooled multi-value features (e.g. genre_ids, 0-padded)
    dense    [V, Dn] float: the item tower's `dense` columns
    """

    def __init__(self, sparse=None, sequence=None, dense=None, device='cuda'):
        dev = torch.device(device)
        self.sparse = _to_device(sparse, dev) if sparse is not None else None
        self.sequence = {k: _to_device(v, dev) for k, v in (sequence or {}).items()}
        self.dense = _to_device(dense, dev, as_float=True) if dense is not None else None
        blocks = [t for t in [self.sparse, self.dense, *self.sequence.values()] if t is not None]
        if not blocks:
            raise ValueError('ItemCatalog needs at least one feature block')
        self.num_items = int(blocks[0].shape[0])
        if any(int(t.shape[0]) != self.num_items for t in blocks):
            raise ValueError('all catalog blocks must have one row per item')
        self.device = dev
        self.err_flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def _gather(self, src, ids, N, B):
        F = int(src.shape[1])
        is_int = src.dtype in (torch.int32, torch.int64)
        out = torch.empty(N * B, F, device=self.device, dtype=torch.int64 if is_int else torch.float32)
        widen = 1 if src.dtype == torch.int32 else 0
        elem = src.element_size()
        _hip.call('rs_catalog_gather', src.data_ptr(), elem, widen, self.num_items, F, int(src.stride(0)),
                  ids.data_ptr(), B, N, int(ids.stride(0)), out.data_ptr(), int(out.stride(0)),
                  self.err_flag.data_ptr(), torch.cuda.current_stream().cuda_stream)
        return out

    def materialize(self, neg_ids: torch.Tensor) -> HardNegativeList:
        """neg_ids [B, N] (device, integer) -> list of N item-tower dicts ([B, ...] each)."""
        _hip.require_device(neg_ids)
        if neg_ids.dim() != 2:
            raise ValueError(f'neg_ids must be [B, N], got {tuple(neg_ids.shape)}')
        ids = neg_ids if neg_ids.dtype == torch.int64 else neg_ids.long()
        ids = ids if ids.stride(1) == 1 else ids.contiguous()
        B, N = int(ids.shape[0]), int(ids.shape[1])
        stacked = {}
        if self.sparse is not None:
            stacked['sparse'] = self._gather(self.sparse, ids, N, B)
        if self.dense is not None:
            stacked['dense'] = self._gather(self.dense, ids, N, B)
        if self.sequence:
            stacked['sequence'] = {k: self._gather(v, ids, N, B) for k, v in self.sequence.items()}
        out = HardNegativeList()
        for n in range(N):
            d = {}
            for k, v in stacked.items():
                if k == 'sequence':
                    d[k] = {name: t[n * B:(n + 1) * B] for name, t in v.items()}
                else:
                    d[k] = v[n * B:(n + 1) * B]
            out.append(d)
        out.stacked = stacked
        return out

    def check_errors(self):
        """Raise IndexError if a materialised id was outside [0, num_items) (host sync)."""
        if int(self.err_flag.item()) != 0:
            self.err_flag.zero_()
            raise IndexError('hard-negative item id outside the catalog')


def attach_hard_negatives(batch: dict, neg_ids: torch.Tensor, catalog: ItemCatalog) -> dict:
    """The `hard_negatives` entry the reference's combined collate leaves as a TODO."""
    batch['hard_negatives'] = catalog.materialize(neg_ids)
    return batch


class NegativeMiner:
    """Hard negatives chosen by the model being trained, on the device, step by step:

        miner = NegativeMiner(model, item_loader, catalog, n=10, skip=0, window=31, refresh_every=200,
                              user_history=history, user_id_col=0)
        loss = train_step(model, batch, optimizer, miner=miner)     # or train_one_epoch(..., miner=miner)

    attach(batch) embeds the catalog into a retrieval.ItemIndex on its first call and every
    `refresh_every` calls after it (ItemIndex.build + set_history + set_filters; between refreshes
    the index is stale on purpose, ANCE-style), then draws n ids per user from the ranks
    [skip, skip + window) of the current user tower's ordering over that index
    (TwoTowerModel.mine_hard_negatives: never the positive, never the user's history, only the
    user's filter) and sets batch['hard_negatives'] = catalog.materialize(ids). A genre filter plus
    the history is the reference's "same-genre unseen" definition; no filter is plain model-mined
    negatives. draw = the miner's call counter, so a run replays from (seed, call number).

    Nothing synchronises: the last count stays on the device (`last_count`), and a flag accumulates
    "some user had count < n" (a pool cut short by history, a filter or duplicate ids; such a user's
    negatives repeat, and an empty pool gives id -1, which the catalog flags). check_errors() reads
    the flag with one sync and warns; the caller decides when."""

    def __init__(self, model, item_loader, catalog, n, skip=0, window=None, refresh_every=1, dtype='bf16',
                 user_history=None, user_id_col=None, filters=None, seed=0, item_id_feature='movie_id_enc',
                 item_id_type='sparse'):
        if int(refresh_every) < 1:
            raise ValueError(f'refresh_every must be at least 1, got {refresh_every}')
        self.model = model
        self.item_loader = item_loader
        self.catalog = catalog
        self.n, self.skip, self.window = int(n), int(skip), window
        self.refresh_every = int(refresh_every)
        self.dtype = dtype
        self.user_history = user_history
        self.user_id_col = user_id_col
        self.filters = filters      # ItemIndex.set_filters' masks; a user's filter goes to attach()
        self.seed = int(seed)
        self.item_id_feature, self.item_id_type = item_id_feature, item_id_type
        self.index = None
        self.calls = 0              # attach() calls so far: the next call's draw
        self.refreshes = 0          # index builds so far
        self.last_count = None      # int32 [B] on the device, of the last attach()
        self._short = torch.zeros(1, dtype=torch.int32, device=catalog.device)

    def refresh(self):
        """Embed the catalog with the current item tower into a fresh index."""
        from recommendsystemproject_amd.retrieval import ItemIndex
        m = getattr(self.model, 'module', self.model)
        self.index = ItemIndex.build(m, self.item_loader, self.catalog.device, dtype=self.dtype,
                                     item_id_feature=self.item_id_feature, item_id_type=self.item_id_type,
                                     keep_fp32=self.dtype == 'fp32')
        if self.user_history is not None:
            self.index.set_history(self.user_history)
        if self.filters is not None:
            self.index.set_filters(self.filters)
        self.refreshes += 1
        return self.index

    def attach(self, batch, user_ids=None, filters=None):
        """Mine this batch's hard negatives and set batch['hard_negatives']; returns the batch.
        user_ids [B] (for the history), else column `user_id_col` of the user tower's sparse block;
        filters: which of the miner's filters each user gets, as ItemIndex.search takes them (an
        id, a name or ids [B]); None with a single filter applies it to everyone."""
        from .training_utils import extract_item_id
        if self.index is None or self.calls % self.refresh_every == 0:
            self.refresh()
        pos = extract_item_id(batch['item_tower'], feature_name=self.item_id_feature, feature_type=self.item_id_type)
        if user_ids is None and self.user_id_col is not None:
            user_ids = batch['user_tower']['sparse'][:, self.user_id_col]
        if filters is None and self.filters is not None:
            if self.index.num_filters != 1:
                raise ValueError(f'NegativeMiner holds {self.index.num_filters} filters: attach(filters=) must '
                                 f'name one, or give an id per user')
            filters = 0  # the miner's one filter, for every user
        m = getattr(self.model, 'module', self.model)
        ids, _, count = m.mine_hard_negatives(batch['user_tower'], self.index, self.n, positive_item_ids=pos,
                                              skip=self.skip, window=self.window, user_ids=user_ids, filters=filters,
                                              seed=self.seed, draw=self.calls)
        self.calls += 1
        self.last_count = count
        torch.maximum(self._short, (count < self.n).any().to(torch.int32).view(1), out=self._short)
        batch['hard_negatives'] = self.catalog.materialize(ids)
        return batch

    def check_errors(self):
        """Warn if, since the last check, some user's pool held fewer than n negatives (one sync)."""
        if int(self._short.item()) != 0:
            self._short.zero_()
            import warnings
            warnings.warn(f'NegativeMiner: a user had fewer than n = {self.n} eligible negatives in the window '
                          f'(repeated, or -1 for none); widen the window or loosen the filter')
            return True
        return False
