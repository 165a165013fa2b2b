"""Data-parallel path: batch-sharded ranks, one all-reduce of the flat gradient,
identical clip + Adam on every rank, parameters broadcast from rank 0.

* CPU (gloo, world_size 2): the oracle computes each rank's shard gradient; our flat-buffer
  all-reduce / broadcast glue (recommendsystemproject_amd.dist) must reproduce the average of the
  per-shard gradients that a single process computes for both shards ("virtual ranks").
* GPU (gloo over 2 processes sharing cuda:0): the full HIP training step under DP equals a
  single-process emulation (sum of the two shards' flat gradients / 2, then clip + Adam).
"""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _cfg():
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'demo.yaml')))
    for t in cfg['two_tower'].values():
        t['dropout'] = 0.0
        t.get('transformer_parameters', {})['dropout'] = 0.0
    u = cfg['two_tower']['user_tower']
    u['sparse_features'][0]['vocab_size'] = 300
    u['sequence_features'][0]['vocab_size'] = 400
    cfg['two_tower']['item_tower']['sparse_features'][0]['vocab_size'] = 400
    return cfg


def _cpu_worker(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    from oracle.twotower_oracle import OracleTrainer, model_state_shapes
    from recommendsystemproject_amd import dist as rdist
    from recommendsystemproject_amd import synth
    from recommendsystemproject_amd.flat import FlatParams
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                          WORLD_SIZE=str(world))
        dist.init_process_group('gloo', rank=rank, world_size=world)
        cfg = _cfg()
        maps = {'user': synth.tower_layout(cfg['two_tower']['user_tower']),
                'item': synth.tower_layout(cfg['two_tower']['item_tower'])}
        shapes = {k: s for k, s, _ in model_state_shapes(cfg)}
        state = synth.make_state(shapes, seed=1)
        batches = [synth.batch_to_torch(synth.make_batch(cfg, 16, seed=40 + r)) for r in range(world)]

        def shard_grads(trainer, b):
            for p in trainer.params():
                p.grad = None
            _, _, _, loss = trainer.forward_loss(b, maps, temperature=0.15)
            loss.backward()
            return [p.grad.detach().clone() for p in trainer.params()]

        tr = OracleTrainer(cfg, state)
        # broadcast: rank 1 starts from different weights and must receive rank 0's
        if rank == 1:
            with torch.no_grad():
                for p in tr.params():
                    p.add_(1.0)
        module = torch.nn.Module()
        module._ps = torch.nn.ParameterList([torch.nn.Parameter(p.detach().clone()) for p in tr.params()])
        rdist.broadcast_model(module)
        with torch.no_grad():
            for p, m in zip(tr.params(), module._ps):
                p.copy_(m)
        g = shard_grads(tr, batches[rank])
        flat = FlatParams([torch.nn.Parameter(t.detach().clone()) for t in tr.params()], torch.device('cpu'))
        with torch.no_grad():
            for i, t in enumerate(g):
                flat.grad_view(i).copy_(t)
        rdist.allreduce_flat_grad(flat.grad)
        avg = [flat.grad_view(i) / world for i in range(len(g))]
        if rank == 0:
            ref = OracleTrainer(cfg, state)  # virtual ranks in one process
            per = [shard_grads(ref, b) for b in batches]
            err = max((a - (sum(x[i] for x in per) / world)).abs().max().item() for i, a in enumerate(avg))
            q.put(('ok', err))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover - surfaced by the parent
        q.put(('err', repr(e)))


def test_dp_allreduce_and_broadcast_gloo_cpu():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_cpu_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = q.get(timeout=240)
    for p in procs:
        p.join(timeout=120)
    assert res[0] == 'ok', res
    assert res[1] < 1e-6, res


def _gpu_worker(rank, world, port, q, lazy=False, pool_max=False, shard=False):
    import sys
    if lazy:
        os.environ['RSYS_LAZY_ROWS'] = '1'  # every lookup table: row-sparse exchange + lazy Adam
    if shard:
        os.environ['RSYS_SHARD_ROWS'] = '1'  # every large table row-sharded (but a max-pooled one)
    sys.path.insert(0, ROOT)
    from oracle.twotower_oracle import model_state_shapes
    from recommendsystemproject_amd import dist as rdist
    from recommendsystemproject_amd import synth
    from recommendsystemproject_amd.flat import ensure_flat
    from recommendsystemproject_amd.optim import Adam
    from recommendsystemproject_amd.project.models.TwoTower.GenericTower import GenericTower
    from recommendsystemproject_amd.project.models.TwoTower.TwoTowerModel import TwoTowerModel
    from recommendsystemproject_amd.project.utils.training_utils import train_step, extract_item_id
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                          WORLD_SIZE=str(world))
        dist.init_process_group('gloo', rank=rank, world_size=world)
        dev = torch.device('cuda:0')
        cfg = _cfg()
        if pool_max:  # the item genre bag max-pooled (GenericTower.py:159-160)
            for f in cfg['two_tower']['item_tower']['sparse_features']:
                if f.get('pooling'):
                    f['pooling'] = 'max'
        maps = {'user': synth.tower_layout(cfg['two_tower']['user_tower']),
                'item': synth.tower_layout(cfg['two_tower']['item_tower'])}
        shapes = {k: s for k, s, _ in model_state_shapes(cfg)}
        state = synth.make_state(shapes, seed=1)

        def build():
            m = TwoTowerModel(GenericTower(cfg, 'user_tower'), GenericTower(cfg, 'item_tower'),
                              maps['user'], maps['item'])
            m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
            return m.to(dev)

        batches = [synth.batch_to_torch(synth.make_batch(cfg, 32, seed=60 + r), dev) for r in range(world)]
        model = build()
        if pool_max:
            f0 = ensure_flat(model)
            gw = model.item_tower.embeddings['genre_ids'].weight
            assert gw._rs_lazy.shard is None  # max-pooled: kept replicated
            if shard:
                assert sum(t.shard is not None for t in f0.lazy) >= 3
        rdist.broadcast_model(model)
        opt = Adam(model.parameters(), lr=1e-3)
        train_step(model, batches[rank], opt, 1.0, 0.15)  # all-reduce inside (dist is active)
        # both towers' gradient buckets were all-reduced inside the backward (dist.overlap)
        assert ensure_flat(model).dp_buckets.launched == 2, ensure_flat(model).dp_buckets.launched
        ensure_flat(model).flush()

        def state_vec(m):  # every parameter of the state dict (sharded tables gathered: a collective);
            # not the BatchNorm running statistics (the emulation's model ran one forward per rank
            # batch), nor the biases whose exact gradient is 0 (a training-mode BatchNorm follows:
            # Adam on fp32 noise, as in test_row_sharded_tables_match_replicated_two_ranks_one_gpu)
            names = {n for n, _ in m.named_parameters()}
            sd = m.state_dict()
            return torch.cat([v.detach().reshape(-1).float() for k, v in sorted(sd.items())
                              if k in names and not k.endswith('feature_bn.bias') and not _bn_invariant_bias(k, sd)])
        dp_w = state_vec(model) if shard else ensure_flat(model).data.detach().clone()
        # more steps: every rank must hold bitwise-identical weights (rows touched by one rank only
        # included: the lazy tables replay them from the exchanged gradient); sharded: the
        # replicated part of the flat buffer
        for s in range(2):
            train_step(model, batches[(rank + s + 1) % world], opt, 1.0, 0.15)
        fm = ensure_flat(model)
        fm.flush()
        w3 = (fm.data[:fm.replicated_numel] if shard else fm.data).detach().clone()
        gathered = [torch.empty_like(w3) for _ in range(world)]
        dist.all_gather(gathered, w3)
        diverged = not torch.equal(gathered[0], gathered[1])
        if rank == 0:
            # single-process emulation: sum of both shards' flat grads, mean, clip + Adam
            with rdist.local_only():
                ref = build()
                f = ensure_flat(ref)
                ropt = Adam(ref.parameters(), lr=1e-3)
                ropt.zero_grad()
                for b in batches:
                    U, I, H = ref(b)
                    loss = ref.compute_loss(U, I, item_ids=extract_item_id(b['item_tower']), temperature=0.15)
                    loss.backward()  # accumulates into the flat gradient
                ropt.grad_scale = 1.0 / world
                ropt.step(clip_max_norm=1.0)
                f.flush()
                ref_w = state_vec(ref) if shard else f.data
            if lazy:
                assert len(f.lazy) >= 3
            d = (ref_w - dp_w).abs()
            tol = 1e-4 if shard else 1e-5
            q.put(('diverged', 0.0) if diverged else ('ok', d.max().item(), int((d > tol).sum()), d.numel()))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        q.put(('err', repr(e)))


@pytest.mark.gpu
@pytest.mark.parametrize('lazy,pool_max,shard', [(False, False, False), (True, False, False), (True, True, False),
                                                (True, True, True)],
                         ids=['dense_tables', 'lazy_tables', 'lazy_max_pooled', 'sharded_with_max_pooled'])
def test_dp_training_step_two_ranks_one_gpu(lazy, pool_max, shard):
    """max_pooled: a max-pooled large table under data parallelism (its arg-max gradient exchanged
    as per-lookup rows, rs_pool_max_grad); sharded: the other large tables row-sharded beside it."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gpu_worker, args=(r, 2, port, q, lazy, pool_max, shard)) for r in range(2)]
    for p in procs:
        p.start()
    res = q.get(timeout=280)
    for p in procs:
        p.join(timeout=120)
    assert res[0] == 'ok', res
    # BN batch statistics are per rank in both runs; only summation order differs. The
    # max-pooled / sharded exchanges sum a row's contributions in another order than the
    # emulation's scatter: Adam's normalised step turns that fp32 rounding into up to +-lr on the
    # rare elements whose gradient is ~0 (as test_row_sharded_tables_match_replicated_two_ranks_one_gpu)
    if not (pool_max or shard):
        assert res[1] < 1e-5, res
    else:
        assert res[1] <= 2 * 1e-3 * 1.01 and res[2] <= max(16, 2e-4 * res[3]), res


# ------------------------------------------------------------------ row-sharded large tables
def _shard_cpu_worker(rank, world, port, q):
    """Row-sharded table bookkeeping on CPU (gloo): the shard layout, the full-table state_dict
    (a collective) and load_state_dict of a full table."""
    import sys
    sys.path.insert(0, ROOT)
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                          WORLD_SIZE=str(world), RSYS_LAZY_ROWS='100', RSYS_SHARD_ROWS='100')
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from recommendsystemproject_amd.flat import ensure_flat, shard_rows, unshard
        V, D = 1003, 8
        torch.manual_seed(5 + rank)  # different per rank: the shards must come from rank 0's table
        m = torch.nn.Module()
        m.embeddings = torch.nn.ModuleDict({'big': torch.nn.Embedding(V, D), 'small': torch.nn.Embedding(50, D)})
        m.lin = torch.nn.Linear(4, 4)
        full0 = m.embeddings['big'].weight.detach().clone()
        dist.broadcast(full0, 0)
        f = ensure_flat(m)
        big = m.embeddings['big'].weight
        t = big._rs_lazy
        ok = t.shard == (world, rank) and tuple(big.shape) == (shard_rows(V, world, rank), D)
        ok &= torch.equal(big.detach(), full0[rank::world])
        ok &= m.embeddings['small'].weight.shape[0] == 50 and not hasattr(m.embeddings['small'].weight, '_rs_lazy')
        ok &= f.replicated_numel < f.numel
        sd = m.state_dict()  # collective
        ok &= tuple(sd['embeddings.big.weight'].shape) == (V, D)
        ok &= torch.equal(sd['embeddings.big.weight'], full0)
        new = torch.randn(V, D, generator=torch.Generator().manual_seed(9))
        sd['embeddings.big.weight'] = new
        m.load_state_dict(sd)
        ok &= torch.equal(big.detach(), new[rank::world])
        parts = [new[r::world] for r in range(world)]
        ok &= torch.equal(unshard(parts, V), new)
        q.put(('ok' if ok else 'mismatch', rank))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        q.put(('err', repr(e)))


def test_row_sharded_table_state_gloo_cpu():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_cpu_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(2)]
    for p in procs:
        p.join(timeout=120)
    assert all(r[0] == 'ok' for r in res), res


def _shard_adam_cpu_worker(rank, world, port, q):
    """Adam.state_dict of a row-sharded table gathers the FULL exp_avg / exp_avg_sq (a collective,
    reference shapes); load_state_dict of a full checkpoint keeps this rank's rows. Plus the
    rank-agreement helpers of the training entry (sync_seed, broadcast_scalar, broadcast_buffers)."""
    import sys
    sys.path.insert(0, ROOT)
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                          WORLD_SIZE=str(world), RSYS_LAZY_ROWS='100', RSYS_SHARD_ROWS='100')
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from recommendsystemproject_amd import dist as rdist
        from recommendsystemproject_amd.flat import ensure_flat
        from recommendsystemproject_amd.optim import Adam
        V, D = 1003, 8
        m = torch.nn.Module()
        m.embeddings = torch.nn.ModuleDict({'big': torch.nn.Embedding(V, D), 'small': torch.nn.Embedding(50, D)})
        m.bn = torch.nn.BatchNorm1d(4)
        f = ensure_flat(m)
        big = m.embeddings['big'].weight
        t = big._rs_lazy
        opt = Adam(m.parameters(), lr=1e-3)
        st = opt._state_for_flat(f)
        g = torch.Generator().manual_seed(3)
        M, Vv = torch.randn(V, D, generator=g), torch.rand(V, D, generator=g)
        o = big._rs_offset
        st['m'][o:o + t.V * D] = M[rank::world].reshape(-1)
        st['v'][o:o + t.V * D] = Vv[rank::world].reshape(-1)
        sd = opt.state_dict()  # collective
        i = [id(p) for p in m.parameters()].index(id(big))
        ok = torch.equal(sd['state'][i]['exp_avg'], M) and torch.equal(sd['state'][i]['exp_avg_sq'], Vv)
        ok &= tuple(sd['state'][i]['exp_avg'].shape) == (V, D)
        # a full checkpoint into a fresh optimizer: this rank's rows land in its flat moments
        sd['state'][i]['exp_avg'] = M * 2
        opt2 = Adam(m.parameters(), lr=1e-3)
        opt2.load_state_dict(sd)
        st2 = opt2._flat_state[id(f)]
        ok &= torch.equal(st2['m'][o:o + t.V * D].view(t.V, D), (M * 2)[rank::world])
        ok &= torch.equal(st2['v'][o:o + t.V * D].view(t.V, D), Vv[rank::world])
        # the entry's agreement helpers
        torch.manual_seed(11 + rank)
        seed = rdist.sync_seed()
        seeds = [None] * world
        dist.all_gather_object(seeds, (seed, torch.randint(0, 1 << 30, (4,)).tolist()))
        ok &= all(s == seeds[0] for s in seeds)
        ok &= rdist.broadcast_scalar(0.25 + rank) == 0.25
        m.bn.running_mean.fill_(float(rank))
        rdist.broadcast_buffers(m)
        ok &= float(m.bn.running_mean.abs().max()) == 0.0
        q.put(('ok' if ok else 'mismatch', rank))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        import traceback
        q.put(('err', repr(e), traceback.format_exc()[-1500:]))


def test_row_sharded_adam_state_and_rank_agreement_gloo_cpu():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_adam_cpu_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(2)]
    for p in procs:
        p.join(timeout=120)
    assert all(r[0] == 'ok' for r in res), res


def test_sharded_loader_equal_batches():
    """Data parallel entry: with drop_last every rank's batches have the same size, also when the
    loader's length is a multiple of the world size (rank W-1 got the short batch)."""
    import sys
    sys.path.insert(0, ROOT)
    from recommendsystemproject_amd.train_twotower import _ShardedLoader

    class Fake:
        def __init__(self, n, B, drop_last):
            self.n, self.B, self.drop_last = n, B, drop_last

        def __len__(self):
            return self.n // self.B if self.drop_last else -(-self.n // self.B)

        def __iter__(self):
            for k in range(len(self)):
                yield min(self.B, self.n - k * self.B)

    for n in (750, 768, 700, 64, 100):
        for W in (2, 4):
            sizes = [list(_ShardedLoader(Fake(n, 64, True), r, W)) for r in range(W)]
            assert all(len(s) == len(sizes[0]) for s in sizes)
            assert all(b == 64 for s in sizes for b in s), (n, W, sizes)
            assert sum(map(len, sizes)) == (n // 64) // W * W


def _bits_checksum(t):
    """A bitwise-sensitive checksum of a float tensor: per 1M-element chunk, the int64 sums of its
    int32 bit patterns and of the patterns weighted by position (any flipped bit changes it)."""
    x = t.detach().reshape(-1).view(torch.int32).to(torch.int64)
    n = x.numel() // (1 << 20) * (1 << 20)
    a = x[:n].view(-1, 1 << 20)
    w = torch.arange(1, (1 << 20) + 1, device=x.device, dtype=torch.int64)
    return torch.cat([a.sum(1), (a * w).sum(1), x[n:].sum().view(1)])


def _c3_gpu_worker(rank, world, port, q):
    """C4's workload on the HIP path: the C3 model at its real table sizes (1M / 10M / 10M rows
    x 128, lazy-exact Adam) data-parallel over 2 ranks sharing cuda:0 (gloo), per-rank batch 4096.
    One DP step against rank 0's single-process emulation (both shards' gradients summed, mean,
    clip + Adam), then two more steps after which the ranks' weights must be bitwise identical."""
    import sys
    sys.path.insert(0, ROOT)
    from recommendsystemproject_amd import dist as rdist
    from recommendsystemproject_amd import synth
    from recommendsystemproject_amd.flat import ensure_flat
    from recommendsystemproject_amd.optim import Adam
    from recommendsystemproject_amd.project.models.TwoTower.GenericTower import GenericTower
    from recommendsystemproject_amd.project.models.TwoTower.TwoTowerModel import TwoTowerModel
    from recommendsystemproject_amd.project.utils.training_utils import extract_item_id, train_step
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                          WORLD_SIZE=str(world))
        dist.init_process_group('gloo', rank=rank, world_size=world)
        dev = torch.device('cuda:0')
        cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'c3.yaml')))
        for t in cfg['two_tower'].values():
            t['dropout'] = 0.0
        maps = {'user': synth.tower_layout(cfg['two_tower']['user_tower']),
                'item': synth.tower_layout(cfg['two_tower']['item_tower'])}
        T, lr = float(cfg['train']['temperature']), float(cfg['train']['learning_rate'])

        def build():
            torch.manual_seed(0)
            with torch.device(dev):
                return TwoTowerModel(GenericTower(cfg, 'user_tower'), GenericTower(cfg, 'item_tower'),
                                     maps['user'], maps['item'])

        batches = [synth.batch_to_torch(synth.make_batch(cfg, 4096, seed=900 + r), dev) for r in range(world)]
        model = build()
        f = ensure_flat(model)
        assert len(f.lazy) == 3 and max(t.V for t in f.lazy) == 10_000_000
        rdist.broadcast_model(model)
        opt = Adam(model.parameters(), lr=lr)
        train_step(model, batches[rank], opt, 1.0, T)  # exchange inside (dist is active)
        f.flush()
        res = None
        if rank == 0:
            dp_w = f.data.detach().clone()
            with rdist.local_only():
                ref = build()
                rf = ensure_flat(ref)
                ropt = Adam(ref.parameters(), lr=lr)
                ropt.zero_grad()
                for b in batches:
                    U, I, H = ref(b)
                    ref.compute_loss(U, I, item_ids=extract_item_id(b['item_tower']), temperature=T).backward()
                ropt.grad_scale = 1.0 / world
                ropt.step(clip_max_norm=1.0)
                rf.flush()
            d = (rf.data - dp_w).abs()
            # summation order of a row's contributions differs (union segment sum vs two calls):
            # fp32 rounding, which Adam's normalised step turns into up to +-lr on elements whose
            # gradient is ~0 -- a handful of the ~54M touched elements
            res = (float(d.max()), int((d > 1e-5).sum()), int((rf.data != dp_w).sum()))
            del ref, rf, ropt, dp_w, d
            torch.cuda.empty_cache()
        for s in range(2):
            train_step(model, batches[(rank + s + 1) % world], opt, 1.0, T)
        f.flush()
        cs = _bits_checksum(f.data)
        cs_all = [torch.empty_like(cs) for _ in range(world)]
        dist.all_gather(cs_all, cs)
        same = all(torch.equal(c, cs_all[0]) for c in cs_all)
        if rank == 0:
            q.put(('ok', same) + res)
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        import traceback
        q.put(('err', repr(e), traceback.format_exc()[-1500:]))


@pytest.mark.gpu
def test_c4_workload_two_ranks_real_tables_one_gpu():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_c3_gpu_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = q.get(timeout=280)
    for p in procs:
        p.join(timeout=120)
    assert res[0] == 'ok', res
    _, same, dmax, off, nonequal = res
    assert same, 'ranks diverged'
    assert off <= 64 and dmax <= 2 * 5e-4 * 1.01, res


def _bn_invariant_bias(k, sd):
    """A Linear bias followed by a training-mode BatchNorm1d (its exact gradient is 0)."""
    head, _, leaf = k.rpartition('.')
    base, _, idx = head.rpartition('.')
    return leaf == 'bias' and idx.isdigit() and f'{base}.{int(idx) + 1}.running_mean' in sd


def _c5_d128_cfg():
    """C5's schema (L = 200 history through the encoder) with the large tables at D = 128 and
    their vocabularies capped to 1M rows (row sharding for C5 at D = 128)."""
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'c5.yaml')))
    for t in cfg['two_tower'].values():
        t['dropout'] = 0.0
        t.get('transformer_parameters', {})['dropout'] = 0.0
        for f in (t.get('sparse_features') or []) + (t.get('sequence_features') or []):
            if f['vocab_size'] >= 1_000_000:
                f['vocab_size'], f['embedding_dim'] = 1_000_000, 128
    return cfg


def _shard_gpu_worker(rank, world, port, q, case='demo'):
    """Two ranks on cuda:0 (gloo): the same three DP steps, once with the large tables
    replicated and once row-sharded (single-id and per-token lookups through the all-to-all row
    exchange, pooled bags through partial bags); the sharded model's state_dict (full tables
    gathered) must match the replicated one. case 'demo': every lookup table lazy, B = 32;
    'c5d128': the C5 schema at D = 128, capped vocabularies, B = 64 per rank."""
    import sys
    if case == 'demo':
        os.environ['RSYS_LAZY_ROWS'] = '1'
    sys.path.insert(0, ROOT)
    from oracle.twotower_oracle import model_state_shapes
    from recommendsystemproject_amd import dist as rdist
    from recommendsystemproject_amd import synth
    from recommendsystemproject_amd.flat import ensure_flat
    from recommendsystemproject_amd.optim import Adam
    from recommendsystemproject_amd.project.models.TwoTower.GenericTower import GenericTower
    from recommendsystemproject_amd.project.models.TwoTower.TwoTowerModel import TwoTowerModel
    from recommendsystemproject_amd.project.utils.training_utils import train_step
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                          WORLD_SIZE=str(world))
        dist.init_process_group('gloo', rank=rank, world_size=world)
        dev = torch.device('cuda:0')
        cfg = _cfg() if case == 'demo' else _c5_d128_cfg()
        B = 32 if case == 'demo' else 64
        maps = {'user': synth.tower_layout(cfg['two_tower']['user_tower']),
                'item': synth.tower_layout(cfg['two_tower']['item_tower'])}
        shapes = {k: s for k, s, _ in model_state_shapes(cfg)}
        state = synth.make_state(shapes, seed=1)
        batches = [synth.batch_to_torch(synth.make_batch(cfg, B, seed=60 + r, edge_cases=True), dev)
                   for r in range(world)]
        out, losses = {}, {}
        for mode in ('replicated', 'sharded'):
            os.environ['RSYS_SHARD_ROWS'] = '1' if mode == 'sharded' else '0'
            m = TwoTowerModel(GenericTower(cfg, 'user_tower'), GenericTower(cfg, 'item_tower'),
                              maps['user'], maps['item'])
            m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
            m = m.to(dev)
            rdist.broadcast_model(m)
            f = ensure_flat(m)
            n_sh = sum(t.shard is not None for t in f.lazy)
            if mode == 'sharded':
                assert n_sh >= (3 if case == 'demo' else 2), n_sh
            opt = Adam(m.parameters(), lr=1e-3)
            losses[mode] = [float(train_step(m, batches[(rank + s) % world], opt, 1.0, 0.15))
                            for s in range(3)]
            out[mode] = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
        if rank == 0:
            worst, off, per, n_el = 0.0, 0, {}, 0
            for k, a in out['replicated'].items():
                b = out['sharded'][k]
                assert a.shape == b.shape, (k, a.shape, b.shape)
                d = (a - b).abs()
                if d.max().item() > 1e-4:
                    per[k] = (d.max().item(), int((d > 1e-4).sum()))
                if k.endswith('feature_bn.bias') or _bn_invariant_bias(k, out['replicated']):
                    continue  # exact gradient 0 (a training-mode BatchNorm follows): Adam on fp32 noise
                worst = max(worst, d.max().item())
                off += int((d > 1e-4).sum())
                n_el += d.numel()
            dl = max(abs(x - y) for x, y in zip(losses['replicated'], losses['sharded']))
            q.put(('ok', worst, off, dl, per, n_el))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        import traceback
        q.put(('err', repr(e), traceback.format_exc()[-1500:]))


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['demo', 'c5d128'])
def test_row_sharded_tables_match_replicated_two_ranks_one_gpu(case):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_gpu_worker, args=(r, 2, port, q, case)) for r in range(2)]
    for p in procs:
        p.start()
    res = q.get(timeout=280)
    for p in procs:
        p.join(timeout=120)
    assert res[0] == 'ok', res
    worst, off, dl, n_el = res[1], res[2], res[3], res[5]
    # the sharded exchanges add each row's contributions in another order (per rank first, then
    # over ranks at the owner): fp32 rounding, which Adam's normalised step turns into up to +-lr
    # per step on the rare elements whose gradient is ~0 -- ~1e-4 of the elements (25 and 33 of
    # 320,494 seen in two runs; a wrong gradient moves thousands), bounded at 2e-4
    assert dl < 1e-5, res
    assert off <= max(16, 2e-4 * n_el) and worst <= 2 * 1e-3 * 3 * 1.01, res


def _eval_after_forward_worker(rank, world, port, q):
    """Two ranks on cuda:0 (gloo), row-sharded lazy tables: a training step, then eval-mode
    lookups outside the training forward -- a no_grad model(batch) (agreed per forward), then
    get_item_embeddings on the SAME item tensors on rank 0 and on copies at new addresses on
    rank 1 (validate()'s item indexing). The forward's address-keyed shape agreement must not
    outlive it (dist.end_forward): otherwise rank 0 would take the stale dims without a
    collective while rank 1 agrees per call, and the all-to-all would hang."""
    import sys
    os.environ['RSYS_LAZY_ROWS'] = '1'
    os.environ['RSYS_SHARD_ROWS'] = '1'
    sys.path.insert(0, ROOT)
    from oracle.twotower_oracle import model_state_shapes
    from recommendsystemproject_amd import dist as rdist
    from recommendsystemproject_amd import synth
    from recommendsystemproject_amd.flat import ensure_flat
    from recommendsystemproject_amd.optim import Adam
    from recommendsystemproject_amd.project.models.TwoTower.GenericTower import GenericTower
    from recommendsystemproject_amd.project.models.TwoTower.TwoTowerModel import TwoTowerModel
    from recommendsystemproject_amd.project.utils.training_utils import train_step
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                          WORLD_SIZE=str(world))
        dist.init_process_group('gloo', rank=rank, world_size=world)
        dev = torch.device('cuda:0')
        cfg = _cfg()
        maps = {'user': synth.tower_layout(cfg['two_tower']['user_tower']),
                'item': synth.tower_layout(cfg['two_tower']['item_tower'])}
        shapes = {k: s for k, s, _ in model_state_shapes(cfg)}
        m = TwoTowerModel(GenericTower(cfg, 'user_tower'), GenericTower(cfg, 'item_tower'),
                          maps['user'], maps['item'])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state(shapes, seed=1).items()})
        m = m.to(dev)
        rdist.broadcast_model(m)
        assert sum(t.shard is not None for t in ensure_flat(m).lazy) >= 3
        opt = Adam(m.parameters(), lr=1e-3)
        train_step(m, synth.batch_to_torch(synth.make_batch(cfg, 32, seed=80 + rank), dev), opt, 1.0, 0.15)
        m.eval()
        b = synth.batch_to_torch(synth.make_batch(cfg, 24, seed=90 + rank), dev)
        with torch.no_grad():
            _, item_fwd, _ = m(b)
            def _copy(x):
                if torch.is_tensor(x):
                    return x.clone()
                return {k: _copy(v) for k, v in x.items()} if isinstance(x, dict) else x
            items = b['item_tower'] if rank == 0 else _copy(b['item_tower'])
            item_idx = m.get_item_embeddings(items)
        torch.cuda.synchronize()
        q.put(('ok', rank, bool(torch.equal(item_fwd, item_idx))))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        import traceback
        q.put(('err', rank, traceback.format_exc()[-1500:]))


@pytest.mark.gpu
def test_eval_lookups_after_forward_row_sharded_two_ranks_one_gpu():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_eval_after_forward_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=200) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
    assert all(r[0] == 'ok' and r[2] for r in res), res


def _overlap_cpu_worker(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    from recommendsystemproject_amd import dist as rdist
    from recommendsystemproject_amd.flat import FlatParams
    from recommendsystemproject_amd.optim import Adam
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                          WORLD_SIZE=str(world))
        dist.init_process_group('gloo', rank=rank, world_size=world)
        torch.manual_seed(0)
        model = torch.nn.Module()
        model.user_tower = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s)) for s in (5, (3, 7), 1)])
        model.item_tower = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s)) for s in ((4, 4), 6)])
        model.extra = torch.nn.Parameter(torch.randn(3))  # in no bucket: reduced at the end
        f = FlatParams(list(model.parameters()), torch.device('cpu'))
        gb = rdist.setup_buckets(model, [model.user_tower, model.item_tower])
        assert gb is not None and len(gb.spans) == 2
        user, item = list(model.user_tower), list(model.item_tower)
        # forward: two ops write the user tower's gradient, one the item tower's
        rdist.note_writer(user[:2])
        rdist.note_writer(user[2:])
        rdist.note_writer(item)
        g = torch.Generator().manual_seed(100 + rank)
        local = torch.randn(f.numel, generator=g)
        with rdist.overlap(model):
            f.grad.copy_(local)
            rdist.note_writer(item, written=True)
            n_item = len(gb.works)
            rdist.note_writer(user[2:], written=True)
            n_mid = len(gb.works)
            rdist.note_writer(user[:2], written=True)
            n_all = len(gb.works)
        opt = Adam.__new__(Adam)
        rdist.allreduce_gradients(model, opt)
        total = torch.zeros_like(local)
        for r in range(world):
            total += torch.randn(f.numel, generator=torch.Generator().manual_seed(100 + r))
        err = (f.grad - total).abs().max().item()
        # a second forward after a bucket's launch (no allreduce_gradients between) is refused
        rdist.note_writer(item)
        with rdist.overlap(model):
            rdist.note_writer(item, written=True)
        refused = False
        try:
            rdist.note_writer(item)
        except RuntimeError:
            refused = True
        rdist.allreduce_gradients(model, opt)
        if rank == 0:
            q.put(('ok', (n_item, n_mid, n_all, err, refused, opt.grad_scale)))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        import traceback
        q.put(('err', traceback.format_exc()))


def test_dp_overlap_buckets_gloo_cpu():
    """dist.GradBuckets: each tower's all-reduce starts when its last gradient writer reports
    (not before), the uncovered rest is reduced by allreduce_gradients, and the sum is exact."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_overlap_cpu_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = q.get(timeout=240)
    for p in procs:
        p.join(timeout=120)
    assert res[0] == 'ok', res
    n_item, n_mid, n_all, err, refused, scale = res[1]
    assert (n_item, n_mid, n_all) == (1, 1, 2)
    assert err < 1e-6 and refused and scale == 0.5


@pytest.mark.gpu
@pytest.mark.parametrize('launcher', ['self', 'torchrun'])
def test_bench_two_ranks_gloo_one_gpu(tmp_path, launcher):
    """bench.py's N > 1 path (one JSON line from rank 0, bucketed all-reduce started in the
    backward, max-over-ranks timing), two gloo ranks sharing the GPU: eager steps (host-staged
    gloo collectives cannot be captured; RCCL runs capture them). 'self': the driver's plain
    `python bench.py --gpus 2` (bench.launch_ranks starts the ranks); 'torchrun': under
    torch.distributed.run."""
    import json
    import subprocess
    import sys
    port = _free_port()
    env = dict(os.environ, RSYS_DIST_BACKEND='gloo', MASTER_ADDR='127.0.0.1')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT'):
        env.pop(k, None)
    args = [os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '3', '--warmup', '2', '--config', 'c2',
            '--full', '--no-cpu-baseline', '--extra=']  # --full: the instrumented eager steps at N > 1 too
    if launcher == 'torchrun':
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
               '--master-addr', '127.0.0.1', '--master-port', str(port)] + args
    else:
        cmd = [sys.executable] + args
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['config']['parallelism'] == 'dp2' and d['value'] > 0
    assert d['config']['hip_graph'] is False


# ------------------------------------------------------------------ per-forward shape agreement
def _agree_cpu_worker(rank, world, port, q):
    """dist.agree_batch: one all-reduce per forward gives every batch tensor's per-dimension
    maxima over the ranks and whether the ranks differ; local_only() issues nothing."""
    import sys
    sys.path.insert(0, ROOT)
    from recommendsystemproject_amd import dist as rdist
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                          WORLD_SIZE=str(world))
        dist.init_process_group('gloo', rank=rank, world_size=world)
        B, L = 8, 5 + 2 * rank  # rank r's history is padded to its own longest list
        batch = {'user_tower': {'sparse': torch.zeros(B, 3, dtype=torch.int64),
                                'sequence': {'hist': torch.zeros(B, L, dtype=torch.int64),
                                             'tags': torch.zeros(B, 4, 3, dtype=torch.int64)}},
                 'item_tower': {'sparse': torch.zeros(B, 2, dtype=torch.int64)}}
        res = {}
        rdist.agree_batch(batch)
        u = batch['user_tower']
        res['hist'] = rdist.agreed_dims(u['sequence']['hist'])
        res['tags'] = rdist.agreed_dims(u['sequence']['tags'])
        res['sparse'] = rdist.agreed_dims(u['sparse'])
        res['static'] = rdist._AGREE.static
        res['other'] = rdist.agreed_dims(torch.zeros(B, L))  # not a batch tensor
        # the lookup call shapes the forward derives (functions._agreed), without a collective
        from recommendsystemproject_amd.functions import _agreed
        res['tokens'] = _agreed(u['sequence']['hist'], tokens=True)
        res['bag'] = _agreed(u['sequence']['tags'], tokens=True)
        rdist.end_forward()  # the forward is over: its address-keyed table is gone
        res['ended'] = rdist.agreed_dims(u['sparse'])
        rdist.clear_agreement()
        res['cleared'] = rdist.agreed_dims(u['sparse'])
        # batches of different structure raise on the fixed-size header, before any vector of
        # rank-dependent length is all-reduced
        odd = dict(batch, extra=torch.zeros(2, dtype=torch.int64)) if rank == 1 else batch
        try:
            rdist.agree_batch(odd)
            res['mismatch'] = None
        except RuntimeError as e:
            res['mismatch'] = 'different tensors' in str(e)
        # equal shapes on every rank: static
        batch['user_tower']['sequence']['hist'] = torch.zeros(B, 9, dtype=torch.int64)
        rdist.agree_batch(batch)
        res['static2'] = rdist._AGREE.static
        with rdist.local_only():  # one rank alone: no collective may be issued
            if rank == 0:
                rdist.agree_batch(batch)
                res['local_agree'] = rdist.agree_max(3, 4)
                res['local_active'] = rdist.is_active()
        res['active'] = rdist.is_active()
        q.put(('ok', rank, res))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        import traceback
        q.put(('err', rank, traceback.format_exc()[-1500:]))


def test_agree_batch_one_allreduce_per_forward_gloo_cpu():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_agree_cpu_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(2)]
    for p in procs:
        p.join(timeout=120)
    assert all(r[0] == 'ok' for r in res), res
    for _, rank, r in res:
        assert r['hist'] == ((8, 7), True), r
        assert r['tags'] == ((8, 4, 3), False) and r['sparse'] == ((8, 3), False), r
        assert r['static'] is False and r['other'] is None and r['cleared'] is None, r
        assert r['ended'] is None and r['mismatch'] is True, r
        assert r['tokens'] == (56, 1, True) and r['bag'] == (32, 3, False), r
        assert r['static2'] is True and r['active'] is True, r
        if rank == 0:
            assert r['local_agree'] == [3, 4] and r['local_active'] is False, r


# ------------------------------------------------------------------ C4's default path at W = 4
def _c3_batch_ids(cfg, maps, batches):
    """Per large table (the C3 schema: user ids, the pooled history, item ids), every id the
    batches look up (int64, unique)."""
    u_col = maps['user']['sparse']['user_id_enc']
    i_col = maps['item']['sparse']['item_id_enc']
    out = {'user_id_enc': [], 'hist_item_ids': [], 'item_id_enc': []}
    for b in batches:
        out['user_id_enc'].append(b['user_tower']['sparse'][:, u_col])
        out['hist_item_ids'].append(b['user_tower']['sequence']['hist_item_ids'].reshape(-1))
        out['item_id_enc'].append(b['item_tower']['sparse'][:, i_col])
    return {k: torch.unique(torch.cat(v).long().cpu()) for k, v in out.items()}


def _c4_w4_worker(rank, world, port, q):
    """C4's workload on the path it takes at W >= 4: the C3 model at its real table sizes (1M /
    10M / 10M rows x 128), every large table row-sharded by default (flat.SHARD_AUTO_WORLD; no
    RSYS_SHARD_ROWS): the single-id user / item features through the all-to-all row exchange, the
    pooled 50-long history through partial bags + reduce-scatter. 4 gloo ranks share cuda:0,
    per-rank batch 4096. One DP step against rank 0's single-process emulation (the 4 batches'
    gradients summed, mean, clip + Adam): every touched row of every shard (sent to rank 0), the
    dense parameters, and a sample of untouched rows; then two more steps after which the dense
    parameters of the ranks are bitwise identical."""
    import sys
    sys.path.insert(0, ROOT)
    os.environ.pop('RSYS_SHARD_ROWS', None)
    from recommendsystemproject_amd import dist as rdist
    from recommendsystemproject_amd import synth
    from recommendsystemproject_amd.flat import SHARD_AUTO_WORLD, ensure_flat
    from recommendsystemproject_amd.optim import Adam
    from recommendsystemproject_amd.project.models.TwoTower.GenericTower import GenericTower
    from recommendsystemproject_amd.project.models.TwoTower.TwoTowerModel import TwoTowerModel
    from recommendsystemproject_amd.project.utils.training_utils import extract_item_id, train_step
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                          WORLD_SIZE=str(world))
        dist.init_process_group('gloo', rank=rank, world_size=world)
        assert world >= SHARD_AUTO_WORLD
        dev = torch.device('cuda:0')
        cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'c3.yaml')))
        for t in cfg['two_tower'].values():
            t['dropout'] = 0.0
        maps = {'user': synth.tower_layout(cfg['two_tower']['user_tower']),
                'item': synth.tower_layout(cfg['two_tower']['item_tower'])}
        T, lr = float(cfg['train']['temperature']), float(cfg['train']['learning_rate'])

        def build():
            torch.manual_seed(0)
            with torch.device(dev):
                return TwoTowerModel(GenericTower(cfg, 'user_tower'), GenericTower(cfg, 'item_tower'),
                                     maps['user'], maps['item'])

        batches = [synth.batch_to_torch(synth.make_batch(cfg, 4096, seed=900 + r), dev) for r in range(world)]
        model = build()
        f = ensure_flat(model)
        names = {id(m.weight): n for tw in (model.user_tower, model.item_tower) for n, m in tw.embeddings.items()
                 if hasattr(m, 'weight')}
        assert len(f.lazy) == 3 and all(t.shard == (world, rank) for t in f.lazy), [t.shard for t in f.lazy]
        rdist.broadcast_model(model)
        opt = Adam(model.parameters(), lr=lr)
        train_step(model, batches[rank], opt, 1.0, T)  # sharded exchanges inside (dist is active)
        f.flush()
        ids = _c3_batch_ids(cfg, maps, batches)
        mine = {}
        for t in f.lazy:
            n = names[id(t.param)]
            own = ids[n][ids[n] % world == rank]
            mine[n] = (own, t.param.detach()[(own // world).to(dev)].cpu())
        res = None
        if rank == 0:
            got = {n: [mine[n]] for n in mine}
            for r in range(1, world):
                for n in sorted(mine):
                    k = torch.zeros(1, dtype=torch.int64)
                    dist.recv(k, r)
                    own = torch.empty(int(k), dtype=torch.int64)
                    rows = torch.empty(int(k), 128)
                    dist.recv(own, r)
                    dist.recv(rows, r)
                    got[n].append((own, rows))
            dense = f.data[:f.dense_numel].clone()
            with rdist.local_only():
                ref = build()
                rf = ensure_flat(ref)
                assert all(t.shard is None for t in rf.lazy)
                ropt = Adam(ref.parameters(), lr=lr)
                ropt.zero_grad()
                for b in batches:
                    U, I, H = ref(b)
                    ref.compute_loss(U, I, item_ids=extract_item_id(b['item_tower']), temperature=T).backward()
                ropt.grad_scale = 1.0 / world
                ropt.step(clip_max_norm=1.0)
                rf.flush()
            rnames = {id(m.weight): n for tw in (ref.user_tower, ref.item_tower) for n, m in tw.embeddings.items()
                      if hasattr(m, 'weight')}
            worst, off, touched, untouched_bad = 0.0, 0, 0, 0
            for t in rf.lazy:
                n = rnames[id(t.param)]
                full = t.param.detach()
                for own, rows in got[n]:
                    d = (full[own.to(dev)].cpu() - rows).abs()
                    worst = max(worst, float(d.max()) if d.numel() else 0.0)
                    off += int((d > 1e-5).sum())
                    touched += own.numel()
                # rank 0's untouched rows (a sample) are the initial rows in both
                sample = torch.arange(0, t.V, 997)
                sample = sample[(sample % world == 0) & ~torch.isin(sample, ids[n])]
                mine_t = [x for x in f.lazy if names[id(x.param)] == n][0]
                untouched_bad += int((mine_t.param.detach()[(sample // world).to(dev)] != full[sample.to(dev)]).sum())
            dd = (rf.data[:rf.dense_numel] - dense).abs()
            res = (worst, off, touched, untouched_bad, float(dd.max()), int((dd > 1e-5).sum()))
            del ref, rf, ropt
            torch.cuda.empty_cache()
        else:
            for n in sorted(mine):
                own, rows = mine[n]
                dist.send(torch.tensor([own.numel()], dtype=torch.int64), 0)
                dist.send(own.contiguous(), 0)
                dist.send(rows.contiguous(), 0)
        dist.barrier()
        for s in range(2):
            train_step(model, batches[(rank + s + 1) % world], opt, 1.0, T)
        cs = _bits_checksum(f.data[:f.dense_numel])
        cs_all = [torch.empty_like(cs) for _ in range(world)]
        dist.all_gather(cs_all, cs)
        same = all(torch.equal(c, cs_all[0]) for c in cs_all)
        if rank == 0:
            q.put(('ok', same) + res)
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        import traceback
        q.put(('err', repr(e), traceback.format_exc()[-2500:]))


@pytest.mark.gpu
def test_c4_workload_four_ranks_row_sharded_real_tables_one_gpu():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_c4_w4_worker, args=(r, 4, port, q)) for r in range(4)]
    for p in procs:
        p.start()
    res = q.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
    assert res[0] == 'ok', res
    _, same, worst, off, touched, untouched_bad, ddmax, dd_off = res
    assert same, 'ranks diverged'
    assert touched > 100_000 and untouched_bad == 0, res
    # each row's contributions are summed in another order (per rank, then at the owner / in the
    # reduce-scatter): fp32 rounding, which Adam's normalised step turns into up to +-lr on the
    # rare elements whose gradient is ~0 (as at W = 2, test_c4_workload_two_ranks_real_tables_one_gpu)
    assert off <= 64 and worst <= 2 * 5e-4 * 1.01, res
    assert dd_off <= 64 and ddmax <= 2 * 5e-4 * 1.01, res


@pytest.mark.gpu
def test_bench_four_ranks_c3_row_sharded_gloo_one_gpu():
    """bench.py --gpus 4 on C3 (C4's configuration): four gloo ranks sharing the GPU, large tables
    row-sharded by default; one JSON line with parallelism dp4 and the sharded-table count."""
    import json
    import subprocess
    import sys
    port = _free_port()
    env = dict(os.environ, RSYS_DIST_BACKEND='gloo', MASTER_ADDR='127.0.0.1')
    env.pop('RSYS_SHARD_ROWS', None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '4',
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.join(ROOT, 'bench.py'),
           '--gpus', '4', '--steps', '2', '--warmup', '1', '--config', 'c3', '--dtype', 'fp32',
           '--full', '--no-cpu-baseline', '--extra=']  # --full: the instrumented pass over the sharded tables
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=560)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 4 and d['config']['parallelism'] == 'dp4' and d['value'] > 0
    assert d['config']['row_sharded_tables'] == 3, d['config']
