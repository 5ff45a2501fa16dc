"""Table-sharded distributed DLRM_Net on the GPU: 2 ranks on ONE MI355X (gloo rendezvous, all-to-all staged
through the host — the RCCL path needs one GPU per rank) against the 2-rank run of the reference
(tests/golden/dist2_tiny.npz): per-rank outputs, losses, DDP-averaged MLP parameters and the reference's
N x embedding-gradient behaviour."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import golden_batches, load_golden, params_with_prefix

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, size, port, q, chunks=1, fixture="dist2_tiny", dense_sync="ddp"):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(size), LOCAL_RANK="0")
    import dlrm_amd
    from dlrm_amd import ext_dist, ops
    d, meta = load_golden(fixture)
    ext_dist.init_distributed(rank=rank, local_rank=0, size=size, use_gpu=True, backend="gloo")
    dev = torch.device("cuda:0")
    np.random.seed(3)
    model = dlrm_amd.DLRM_Net(meta["m_spa"], np.asarray(meta["ln_emb"]), np.asarray(meta["ln_bot"]), np.asarray(meta["ln_top"]),
                              "dot", sigmoid_top=meta["sigmoid_top"], loss_function="bce")
    init = params_with_prefix(d, "init")
    with torch.no_grad():
        for j, g in enumerate(model.local_emb_indices):
            model.emb_l[j].weight.copy_(torch.from_numpy(init[f"emb_l.{g}.weight"]))
        for name, p in model.bot_l.named_parameters():
            p.copy_(torch.from_numpy(init[f"bot_l.{name}"]))
        for name, p in model.top_l.named_parameters():
            p.copy_(torch.from_numpy(init[f"top_l.{name}"]))
    model = model.to(dev)
    model.emb_update_mode = ops.UPD_DETERMINISTIC
    model.a2a_chunks = chunks                # > 1: pipelined all-to-all (DLRM_Net._pipelined_exchange_forward)
    wrap = ext_dist.FlatDDP if dense_sync == "flat" else ext_dist.DDP
    model.bot_l = wrap(model.bot_l, device_ids=[0])
    model.top_l = wrap(model.top_l, device_ids=[0])
    opt = torch.optim.SGD([{"params": [p for e in model.emb_l for p in e.parameters()], "lr": meta["lr"]},
                           {"params": model.bot_l.parameters(), "lr": meta["lr"]},
                           {"params": model.top_l.parameters(), "lr": meta["lr"]}], lr=meta["lr"])
    res = {}
    for s, (X, lS_o, lS_i, T) in enumerate(golden_batches(d, meta)):
        Z = model(torch.from_numpy(X).to(dev), torch.stack([torch.from_numpy(o) for o in lS_o]).to(dev),
                  [torch.from_numpy(i).to(dev) for i in lS_i])
        Tl = torch.from_numpy(T)[ext_dist.get_my_slice(T.shape[0])].to(dev)
        E = model.loss_fn(Z, Tl)
        res[f"s{s}.Z"] = Z.detach().cpu().numpy()
        res[f"s{s}.loss"] = float(E.detach())
        opt.zero_grad()
        E.backward()
        if dense_sync == "flat":
            # the weight-gradient GEMMs wrote straight into the flat all-reduce buffers: no gradient was copied
            for tower in (model.bot_l, model.top_l):
                assert all(p.grad.data_ptr() == tower._view(i).data_ptr() for i, p in enumerate(tower._params))
        opt.step()
    torch.cuda.synchronize()
    for j, g in enumerate(model.local_emb_indices):
        res[f"final.emb_l.{g}.weight"] = model.emb_l[j].weight.detach().cpu().numpy()
    for name, p in model.bot_l.module.named_parameters():
        res[f"final.bot_l.{name}"] = p.detach().cpu().numpy()
    for name, p in model.top_l.module.named_parameters():
        res[f"final.top_l.{name}"] = p.detach().cpu().numpy()
    q.put((rank, res))
    ext_dist.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("fixture,chunks,dense_sync", [("dist2_tiny", 1, "ddp"), ("dist2_tiny", 2, "ddp"), ("dist8_t26", 1, "ddp"),
                                                       ("dist8_t26", 2, "ddp"), ("dist2_tiny", 1, "flat"), ("dist8_t26", 2, "flat")],
                         ids=["2ranks-single-exchange", "2ranks-pipelined-2-chunks", "8ranks-26tables-single-exchange",
                              "8ranks-26tables-pipelined-2-chunks", "2ranks-flat-allreduce", "8ranks-26tables-pipelined-flat-allreduce"])
def test_multi_rank_training_matches_reference_multi_rank_run(fixture, chunks, dense_sync):
    """dist8_t26: the real Criteo partition — 26 tables over 8 ranks ([4,4,3,3,3,3,3,3]), B = 64 (8 per rank) — through
    DLRM_Net.distributed_forward, ext_dist.alltoall() and DDP (or ext_dist.FlatDDP: one flat gradient buffer the weight-gradient
    GEMMs write into, one all-reduce per tower), against the reference's own 8-rank run."""
    d, meta = load_golden(fixture)
    size = meta["size"]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, size, port, q, chunks, fixture, dense_sync)) for r in range(size)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=600) for _ in range(size))
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for r in range(size):
        for s in range(meta["steps"]):
            np.testing.assert_allclose(results[r][f"s{s}.Z"], d[f"rank{r}.s{s}.Z"], rtol=2e-5, atol=1e-6)
            want = float(d[f"rank{r}.s{s}.loss"])
            assert abs(results[r][f"s{s}.loss"] - want) <= 1e-5 * abs(want)
        for k, v in results[r].items():
            if k.startswith("final.emb_l"):
                np.testing.assert_allclose(v, d[f"rank{r}.{k}"], rtol=1e-4, atol=2e-6, err_msg=k)
            elif k.startswith("final."):
                np.testing.assert_allclose(v, d[f"rank0.{k}"], rtol=1e-4, atol=2e-6, err_msg=k)


# ---------------------------------------------------------------------------------------------------------------------
# BASELINE configs[3] AT ITS OWN SHAPES: T = 26, D = 128, towers 13-512-256-128 / 479-1024-1024-512-256-1, global B = 65536
# (8192 per rank), 8 ranks -> tables [4,4,3,3,3,3,3,3] — against the reference's own 8-rank run (tests/golden/dist8_tb.npz,
# oracle/make_golden.py dist8tb; dlrm_s_pytorch.py:528-585, extend_distributed.py:541-576)
# ---------------------------------------------------------------------------------------------------------------------
def _tb_worker(rank, size, port, q, chunks, dense_sync):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(size), LOCAL_RANK="0")
    import dlrm_amd
    import golden_tb
    from dlrm_amd import ext_dist, ops
    fx = golden_tb.load("dist8_tb", verify=(rank == 0))
    meta = fx.meta
    ext_dist.init_distributed(rank=rank, local_rank=0, size=size, use_gpu=True, backend="gloo")
    dev = torch.device("cuda:0")
    np.random.seed(3)
    model = dlrm_amd.DLRM_Net(meta["m_spa"], np.asarray(meta["ln_emb"]), np.asarray(meta["ln_bot"]), np.asarray(meta["ln_top"]),
                              "dot", sigmoid_top=meta["sigmoid_top"], loss_function="bce")
    with torch.no_grad():
        for j, g in enumerate(model.local_emb_indices):
            model.emb_l[j].weight.copy_(torch.from_numpy(fx.init[f"emb_l.{g}.weight"]))
        for name, p in model.bot_l.named_parameters():
            p.copy_(torch.from_numpy(fx.init[f"bot_l.{name}"]))
        for name, p in model.top_l.named_parameters():
            p.copy_(torch.from_numpy(fx.init[f"top_l.{name}"]))
    model = model.to(dev)
    model.emb_update_mode = ops.UPD_SORTED            # the benchmark's update (bit-exact per row where a run stays inside one chunk)
    model.a2a_chunks = chunks
    wrap = ext_dist.FlatDDP if dense_sync == "flat" else ext_dist.DDP
    model.bot_l = wrap(model.bot_l, device_ids=[0])
    model.top_l = wrap(model.top_l, device_ids=[0])
    lr = meta["lr"]
    opt = torch.optim.SGD([{"params": [p for e in model.emb_l for p in e.parameters()], "lr": lr},
                           {"params": model.bot_l.parameters(), "lr": lr}, {"params": model.top_l.parameters(), "lr": lr}], lr=lr)
    res = {}
    for s, (X, off, idx, T) in enumerate(fx.batches):
        Z = model(torch.from_numpy(X).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(idx).to(dev))
        Tl = torch.from_numpy(T)[ext_dist.get_my_slice(T.shape[0])].to(dev)
        E = model.loss_fn(Z, Tl)
        res[f"s{s}.Z"] = Z.detach().cpu().numpy()
        res[f"s{s}.loss"] = float(E.detach())
        opt.zero_grad()
        E.backward()
        if s == 0 and rank == 0:
            res["s0.top8_weight_grad"] = model.top_l.module[8].weight.grad.detach().cpu().numpy()
            res["s0.bot0_bias_grad"] = model.bot_l.module[0].bias.grad.detach().cpu().numpy()
        opt.step()
    torch.cuda.synchronize()
    ops.check_index_errors(sync=True)
    for j, g in enumerate(model.local_emb_indices):
        v = model.emb_l[j].weight.detach().cpu().numpy()
        res[f"final_head.emb_l.{g}.weight"], res[f"final_tail.emb_l.{g}.weight"] = v[:48], v[-48:]
        res[f"final_colsum.emb_l.{g}.weight"] = v.astype(np.float64).sum(0)
        res[f"final_touched.emb_l.{g}.weight"] = v[fx.batches[0][2][g][:64]]
    if rank == 0:
        for tower, mod in (("bot_l", model.bot_l.module), ("top_l", model.top_l.module)):
            for name, p in mod.named_parameters():
                res[f"final.{tower}.{name}"] = p.detach().cpu().numpy()
    res["local_emb_indices"] = list(model.local_emb_indices)
    q.put((rank, res))
    ext_dist.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("chunks,dense_sync", [(1, "ddp"), (2, "flat")], ids=["single-exchange-ddp", "pipelined-2-chunks-flat-allreduce"])
def test_eight_rank_terabyte_shapes_match_the_reference_eight_rank_run(chunks, dense_sync):
    """Config 4 at config-4 shapes: every rank pools the WHOLE 65536-sample batch for its 3-4 tables (D = 128), one all-to-all turns
    [B, T_loc*D] into 8 blocks [8192, T_s*D]; the D = 128 LDS-DMA interaction reads x + those eight receive blocks (widths
    4,4,3,3,3,3,3,3) and its backward writes into the chunks of the reverse exchange's send buffer; towers 13-512-256-128 /
    479-1024-1024-512-256-1 under DDP / FlatDDP.  All 8 ranks share ONE MI355X here (gloo rendezvous, host-staged exchange): the
    bookkeeping, layouts and kernels are the real ones, only the transport is not RCCL.  Compared with the reference's own 8-rank
    gloo run: per-rank predictions (rtol 2e-5), per-rank losses (1e-5), two step-0 gradients after the all-reduce, final towers
    and final tables (rtol 1e-4; every 8th row + fp64 row / column sums for the large matrices, as the fixture stores them)."""
    import golden_tb
    fx = golden_tb.load("dist8_tb")
    d, meta = fx.d, fx.meta
    size = meta["size"]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_tb_worker, args=(r, size, port, q, chunks, dense_sync)) for r in range(size)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=900) for _ in range(size))
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    split = [4, 4, 3, 3, 3, 3, 3, 3]
    for r in range(size):
        assert results[r]["local_emb_indices"] == list(range(sum(split[:r]), sum(split[:r + 1]))) == d[f"rank{r}.local_emb_indices"].tolist()
        for s in range(meta["steps"]):
            assert results[r][f"s{s}.Z"].shape == (meta["B"] // size, 1)
            np.testing.assert_allclose(results[r][f"s{s}.Z"], d[f"rank{r}.s{s}.Z"], rtol=2e-5, atol=1e-6)
            want = float(d[f"rank{r}.s{s}.loss"])
            assert abs(results[r][f"s{s}.loss"] - want) <= 1e-5 * abs(want), (r, s)
        for k, v in results[r].items():
            if k.startswith(("final_head.", "final_tail.", "final_touched.")):
                np.testing.assert_allclose(v, d[f"rank{r}.{k}"], rtol=1e-4, atol=2e-6, err_msg=f"rank {r} {k}")
            elif k.startswith("final_colsum."):
                ref = d[f"rank{r}.{k}"]
                np.testing.assert_allclose(v, ref, rtol=1e-4, atol=1e-5 * max(1.0, float(np.abs(ref).max())), err_msg=f"rank {r} {k}")
    r0 = results[0]
    for k in ("s0.top8_weight_grad", "s0.bot0_bias_grad"):
        ref = d[f"rank0.{k}"]
        # a bias gradient of 8192 x 8 cancelling terms: one pre-activation within rounding of zero falls on either side of the ReLU
        # threshold and a whole term appears / disappears — compared on the scale of the tensor (the rule of tests/golden_tb.py)
        np.testing.assert_allclose(r0[k], ref, rtol=2e-4, atol=1e-2 * float(np.abs(ref).max()), err_msg=k)
    n_checked = 0
    for k, v in r0.items():
        if not k.startswith("final.") :
            continue
        name = k[len("final."):]
        if f"rank0.final.{name}" in d:
            np.testing.assert_allclose(v, d[f"rank0.final.{name}"], rtol=1e-4, atol=2e-6, err_msg=k)
        else:
            np.testing.assert_allclose(v[::8], d[f"rank0.final_rows8.{name}"], rtol=1e-4, atol=2e-6, err_msg=k)
            for tag, ax in (("colsum", 0), ("rowsum", 1)):
                ref = d[f"rank0.final_{tag}.{name}"]
                np.testing.assert_allclose(v.astype(np.float64).sum(ax), ref, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(ref).max())),
                                           err_msg=f"{k} {tag}")
        n_checked += 1
    assert n_checked == 16          # 3 + 5 Linear layers, weight + bias


# ---------------------------------------------------------------------------------------------------------------------
# planned sharding (table-wise + row-wise), non-replicated key-major inputs
# ---------------------------------------------------------------------------------------------------------------------
_SH2 = dict(rows=[50, 7, 3000, 11, 400], hot=[3, 1, 7, 2, 1], D=16, dense_in=13, dense=[32, 16], over=[48, 24, 1], B=32, lr=0.2)
# 4 ranks: nine tables, the 9-hot 3000-row table row-wise over all four ranks, two table-wise tables on every rank
_SH4 = dict(rows=[50, 7, 3000, 11, 400, 23, 90, 64, 31], hot=[3, 1, 9, 2, 1, 2, 1, 2, 1], D=16, dense_in=13, dense=[32, 16], over=[48, 24, 1],
            B=32, lr=0.2)
_SH = _SH2


def _sh(size):
    return _SH4 if size == 4 else _SH2


def _sharded_inputs(step, size=2):
    rng = np.random.default_rng(100 + step)
    c = _sh(size)
    X = rng.random((c["B"], c["dense_in"])).astype(np.float32)
    ids = [rng.integers(0, n, size=(c["B"], h)).astype(np.int32) for n, h in zip(c["rows"], c["hot"])]    # [B, h_t] per table
    labels = rng.integers(0, 2, size=c["B"]).astype(np.float32)
    return X, ids, labels


def _sharded_worker(rank, size, port, q, full_init):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(size), LOCAL_RANK="0")
    from dlrm_amd import ext_dist, ops, sharding
    from dlrm_amd.optim import FusedSGD
    from dlrm_amd.torchrec_variant import DLRMTrain, ShardedDLRM
    ext_dist.init_distributed(rank=rank, local_rank=0, size=size, use_gpu=True, backend="gloo")
    dev = torch.device("cuda:0")
    c = _sh(size)
    # force one row-wise table (3000 rows, 7- / 9-hot) plus planned table-wise placement of the rest
    plan = sharding.plan(c["rows"], c["hot"], c["D"], size, c["B"], row_wise_threshold=0.6)
    assert plan.row_wise() == [2], plan
    np.random.seed(1)
    model = ShardedDLRM(c["rows"], c["hot"], c["D"], c["dense_in"], c["dense"], c["over"], c["B"], plan=plan)
    model.load_full_state(full_init)
    model = model.to(dev)
    model.emb_update_mode = ops.UPD_DETERMINISTIC
    model.bot_l = ext_dist.DDP(model.bot_l, device_ids=[0])
    model.top_l = ext_dist.DDP(model.top_l, device_ids=[0])
    train = DLRMTrain(model)
    opt = FusedSGD([{"params": [p for e in model.emb_l for p in e.parameters()], "lr": c["lr"]},
                    {"params": model.bot_l.parameters(), "lr": c["lr"]}, {"params": model.top_l.parameters(), "lr": c["lr"]}], lr=c["lr"])
    Bl = c["B"] // size
    sl = slice(rank * Bl, (rank + 1) * Bl)
    res = {}
    for s in range(2):
        X, ids, labels = _sharded_inputs(s, size)
        values = torch.from_numpy(np.concatenate([i[sl].reshape(-1) for i in ids])).to(dev)       # key-major ids of MY samples only
        loss, (_, logits, _) = _train_step(train, torch.from_numpy(X[sl]).to(dev), values, torch.from_numpy(labels[sl]).to(dev))
        res[f"s{s}.logits"] = logits.cpu().numpy()
        res[f"s{s}.loss"] = float(loss)
        opt.zero_grad()
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    ops.check_index_errors(sync=True)
    j = 0
    for t in model.tw_mine:
        res[f"final.emb.{t}"] = (0, model.emb_l[j].weight.detach().cpu().numpy()); j += 1
    for t in model.rw_tables:
        res[f"final.emb.{t}"] = (model.rw_range[t][0], model.emb_l[j].weight.detach().cpu().numpy()); j += 1
    for name, p in model.top_l.module.named_parameters():
        res[f"final.top_l.{name}"] = p.detach().cpu().numpy()
    res["tw_mine"], res["feature_order"] = list(model.tw_mine), list(model.feature_order)
    q.put((rank, res))
    ext_dist.barrier()
    torch.distributed.destroy_process_group()


def _train_step(train, dense, values, labels):
    """DLRMTrain.forward for the sharded model: forward(dense, values) -> logits"""
    logits = train.model(dense, values)
    loss = train.loss_fn(logits, labels.to(torch.float32).reshape(logits.shape))
    return loss, (loss.detach(), logits.detach(), labels)


@pytest.mark.parametrize("size", [2, 4])
def test_sharded_dlrm_ranks_match_single_process_oracle(size):
    """ShardedDLRM on 2 and 4 ranks (one MI355X, gloo rendezvous): table-wise + one ROW-WISE table, each rank feeding only its slice of
    the batch — against the single-process oracle on the whole batch: logits of every rank's slice, per-rank losses (mean over
    the local slice), and after two steps the embedding shards (the reference's N x embedding-gradient behaviour: oracle
    emb_lr_scale = N) and the DDP-averaged top tower."""
    from oracle import oracle as O
    c = _sh(size)
    rng = np.random.default_rng(9)
    T = len(c["rows"])
    F = T + 1
    ln_bot, ln_top = [c["dense_in"]] + c["dense"], [c["D"] + F * (F - 1) // 2] + c["over"]
    full = {}
    for t, n in enumerate(c["rows"]):
        full[f"emb_l.{t}.weight"] = (rng.standard_normal((n, c["D"])) * 0.2).astype(np.float32)
    for name, ln in (("bot_l", ln_bot), ("top_l", ln_top)):
        for i in range(len(ln) - 1):
            full[f"{name}.{2 * i}.weight"] = (rng.standard_normal((ln[i + 1], ln[i])) / np.sqrt(ln[i])).astype(np.float32)
            full[f"{name}.{2 * i}.bias"] = (rng.standard_normal(ln[i + 1]) * 0.1).astype(np.float32)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sharded_worker, args=(r, size, port, q, full)) for r in range(size)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=600) for _ in range(size))
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    ref = O.OracleDLRM(full, pair_order="triu", final_top_act_none=True, loss="bce_logits")
    Bl = c["B"] // size
    for s in range(2):
        X, ids, labels = _sharded_inputs(s, size)
        off = [np.arange(c["B"], dtype=np.int64) * h for h in c["hot"]]
        idx = [i.reshape(-1).astype(np.int64) for i in ids]
        # the distributed loss is the mean over each rank's slice; the global-mean step with emb lr x N reproduces its updates
        Z = ref.forward(X, off, idx)
        for r in range(size):
            sl = slice(r * Bl, (r + 1) * Bl)
            np.testing.assert_allclose(results[r][f"s{s}.logits"], Z[sl], rtol=2e-5, atol=2e-6)
            want, _ = ref._loss(Z[sl], labels[sl].reshape(-1, 1))
            assert abs(results[r][f"s{s}.loss"] - want) <= 1e-5 * abs(want)
        ref.train_step(X, off, idx, labels.reshape(-1, 1), c["lr"], emb_lr_scale=float(size))
    seen = set()
    for r in range(size):
        for k, v in results[r].items():
            if k.startswith("final.emb."):
                t = int(k.split(".")[-1])
                lo, w = v
                np.testing.assert_allclose(w, ref.p[f"emb_l.{t}.weight"][lo:lo + w.shape[0]], rtol=1e-4, atol=5e-6, err_msg=f"rank {r} {k}")
                seen.add((t, lo))
            elif k.startswith("final.top_l."):
                np.testing.assert_allclose(v, ref.p[k[len("final."):]], rtol=1e-4, atol=5e-6, err_msg=k)
    assert len({t for t, _ in seen}) == T and len([1 for t, _ in seen if t == 2]) == size   # the row-wise table came back in one shard per rank


# ---------------------------------------------------------------------------------------------------------------------
# bench.py --gpus 2: the whole N > 1 control flow on ONE GPU (gloo, both ranks on cuda:0, reduced sizes) — not a measurement
# ---------------------------------------------------------------------------------------------------------------------
def _run_bench_n2(extra_env, extra_args, timeout):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DLRM_BENCH_SELFTEST_GLOO="1", **extra_env)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--warmup", "1", "--batch", "4096",
           "--row-cap", "50000"] + extra_args
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and lines, (r.returncode, r.stderr[-3000:])
    return json.loads(lines[-1]), r.stderr


@pytest.mark.parametrize("dense_sync", ["ddp", "flat"])
def test_bench_two_rank_control_flow(dense_sync):
    """headline (reference exchange schedule) + alternative exchange schedule + the other dense-gradient synchronisation + collective
    timings + process-group report, end to end through torchrun, as the driver launches it"""
    d, _ = _run_bench_n2({}, ["--steps", "3", "--hang-timeout", "120", "--dense-sync", dense_sync, "--alts", "--full"], 600)
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["scaling"] == "strong" and "selftest" in d
    assert dense_sync in d["config"]["parallelism"] and d["config"]["a2a_chunks"] == 1
    assert d["alt_a2a_pipelined"]["value"] > 0 and d["alt_a2a_pipelined"]["a2a_chunks"] > 1
    other = d["alt_dense_sync"]
    assert other.get("dense_sync") == ("flat" if dense_sync == "ddp" else "ddp") and other["value"] > 0, other
    # same model, same batches, same arithmetic: the alternative schedules train to the same loss
    assert abs(other["final_loss"] - d["alt_a2a_pipelined"]["final_loss"]) < 5e-3
    assert d["distributed"]["world_size"] == 2 and d["collectives"].get("allreduce_ms", 0) > 0
    assert "linear_fwd" in d["kernels"] and d["roofline"] is not None


def test_update_in_backward_is_inert_under_the_distributed_forward():
    """DLRM_Net.update_in_backward (ABI 17, opt-in) belongs to the single-process fused lookup + interaction path; with table-wise shards the
    lookups run through dlrm_emb_fwd and the all-to-all (distributed_forward, dlrm_s_pytorch.py:528-585) and the switch changes nothing:
    the two-rank run trains, and the line names the reference loop's update schedule."""
    d, _ = _run_bench_n2({"DLRM_UPDATE_IN_BACKWARD": "1"}, ["--steps", "2", "--hang-timeout", "120"], 600)
    assert d["n_gpus"] == 2 and d["value"] > 0 and np.isfinite(d["final_loss"])
    assert d["config"]["sparse_update_schedule"].startswith("every row at optimizer.step()")


def test_bench_two_rank_self_launch_with_bf16_lean_towers_and_flat_allreduce():
    """`python bench.py --gpus 2` WITHOUT a launcher (VERDICT r3 missing-3): bench.py re-executes itself under torch.distributed.run and the
    line says n_gpus 2.  Run with `--mlp-arith bf16 --dense-sync flat`: the lean bf16 towers (bf16-only hidden activations, weight gradient from
    the stored bf16 operands) write their gradients into FlatDDP's flat all-reduce buffers — the combination no other test exercises."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(DLRM_BENCH_SELFTEST_GLOO="1", MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "4096", "--row-cap", "50000",
                        "--hang-timeout", "120", "--mlp-arith", "bf16", "--dense-sync", "flat", "--alts"], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and lines, (r.returncode, r.stderr[-3000:])
    d = json.loads(lines[-1])
    assert "re-executing" in r.stderr and "--nproc-per-node=2" in r.stderr
    assert d["n_gpus"] == 2 and d["dtype"] == "bf16" and "flat" in d["config"]["parallelism"] and np.isfinite(d["final_loss"]) and d["final_loss"] < 1.0
    assert abs(d["alt_dense_sync"]["final_loss"] - d["final_loss"]) < 2e-2          # torch DDP on the same towers trains to the same loss


def test_bench_two_rank_sharded_multihot_control_flow():
    """VERDICT r2 #8 / SURVEY 8 f-3: `bench.py --gpus 2 --workload mlperf_v2_multihot` — planned sharding (ShardedDLRM), per-rank input
    slices through kjt_input_dist (id re-layouts as block-copy kernels), fused row-wise Adagrad, DDP towers — end to end through
    torchrun as the driver launches it (one GPU, gloo rendezvous, reduced sizes: control flow, not a measurement)."""
    d, _ = _run_bench_n2({}, ["--steps", "3", "--hang-timeout", "120", "--workload", "mlperf_v2_multihot", "--interaction", "dot",
                              "--mlp-arith", "f32", "--full"], 600)
    assert d["n_gpus"] == 2 and d["value"] > 0 and "selftest" in d and np.isfinite(d["final_loss"])
    assert "planned sharding x2" in d["config"]["parallelism"] and d["config"]["optimizer"] == "rwsadagrad"
    dist = d["distributed"]
    assert dist["world_size"] == 2 and sum(dist["tables_per_rank"]) + len(dist["row_wise_tables"]) == 26
    assert dist["plan_imbalance"] <= dist["reference_block_partition_imbalance"] + 1e-9
    assert "emb_fwd" in d["kernels"] and "emb_bwd_adagrad" in d["kernels"]


def test_bench_prints_its_headline_when_an_optional_measurement_hangs():
    """DLRM_BENCH_SELFTEST_HANG=alt blocks inside the optional dense-sync measurement: the watchdog must print the finished headline
    line (marked "incomplete") and exit 0 instead of losing the run"""
    d, err = _run_bench_n2({"DLRM_BENCH_SELFTEST_HANG": "alt"}, ["--steps", "1", "--hang-timeout", "3", "--alts"], 300)
    assert d["value"] > 0 and "incomplete" in d and "alt_dense_sync" not in d
    assert "watchdog expired" in err
