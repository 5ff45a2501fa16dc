"""CPU-only checks: the C-ABI library loads and exports every symbol include/dlrm_hip.h declares, the
drop-in module has the reference's surface, host bookkeeping is bit-exact, and the product path refuses
to run without a GPU instead of falling back."""
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden, params_with_prefix


def header_functions():
    src = open(os.path.join(ROOT, "include", "dlrm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dlrm_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from dlrm_amd import _lib
    lib = _lib.load()
    names = header_functions()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
    assert set(_lib.SIGNATURES) == set(names)
    assert lib.dlrm_hip_abi_version() == _lib.EXPECTED_ABI == 17
    assert b"gfx950" in lib.dlrm_hip_build_info()


def test_no_cpu_fallback():
    from dlrm_amd import ops
    W = [torch.zeros(4, 4)]
    with pytest.raises(RuntimeError, match="GPU"):
        ops.BagBatch([torch.zeros(2, dtype=torch.int64)], [torch.zeros(2, dtype=torch.int64)])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.linear_fwd(torch.zeros(2, 2), torch.zeros(2, 2), None, 0, torch.zeros(2, 2))


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "dlrm_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            assert "oracle" not in open(os.path.join(pkg, f)).read().replace("# oracle", ""), f


def test_module_surface_and_rng_order_match_reference():
    """same numpy seed -> bit-identical initial parameters and the reference's state_dict keys"""
    import dlrm_amd
    d, meta = load_golden("config1_b128")
    np.random.seed(123)
    m = dlrm_amd.DLRM_Net(meta["m_spa"], np.asarray(meta["ln_emb"]), np.asarray(meta["ln_bot"]), np.asarray(meta["ln_top"]),
                          arch_interaction_op="dot", sigmoid_top=meta["sigmoid_top"], loss_function="bce")
    init = params_with_prefix(d, "init")
    sd = m.state_dict()
    assert list(sd.keys()) == list(init.keys())
    for k, v in init.items():
        assert np.array_equal(sd[k].numpy(), v), k
    for attr in ("emb_l", "v_W_l", "bot_l", "top_l", "loss_fn", "ndevices", "loss_threshold", "weighted_pooling",
                 "quantize_emb", "apply_mlp", "apply_emb", "interact_features", "create_emb", "create_mlp",
                 "sequential_forward", "distributed_forward"):
        assert hasattr(m, attr), attr
    assert isinstance(m.top_l, torch.nn.Sequential) and isinstance(m.top_l[0], torch.nn.Linear) and len(m.top_l) == 6
    assert all(p.requires_grad for p in m.parameters())
    empty = dlrm_amd.DLRM_Net()
    assert len(list(empty.parameters())) == 0


def test_ext_dist_partition_bit_exact():
    from dlrm_amd import ext_dist
    with open(os.path.join(GOLDEN, "bookkeeping.json")) as f:
        book = json.load(f)
    saved = (ext_dist.my_rank, ext_dist.my_size)
    try:
        for case in book["partition"]:
            for rank, want in enumerate(case["ranks"]):
                ext_dist.my_rank, ext_dist.my_size = rank, case["size"]
                sl = ext_dist.get_my_slice(case["n"])
                assert [sl.start, sl.stop, sl.step] == want["slice"]
                mine, splits = ext_dist.get_split_lengths(case["n"])
                assert mine == want["my_len"] and splits == want["splits"]
    finally:
        ext_dist.my_rank, ext_dist.my_size = saved


def test_error_strings_match_reference():
    import dlrm_amd
    np.random.seed(0)
    with pytest.raises(SystemExit, match="--loss-function=huber is not supported"):
        dlrm_amd.DLRM_Net(2, np.asarray([4, 3]), np.asarray([4, 2]), np.asarray([5, 1]), "dot", loss_function="huber")
    m = dlrm_amd.DLRM_Net(2, np.asarray([4, 3]), np.asarray([4, 2]), np.asarray([5, 1]), "foo")
    with pytest.raises(SystemExit, match="--arch-interaction-op=foo is not supported"):
        m.interact_features(torch.zeros(1, 2), [torch.zeros(1, 2)])


REFERENCE = os.environ.get("DLRM_REFERENCE", "/root/reference")


@pytest.mark.skipif(not os.path.isfile(os.path.join(REFERENCE, "dlrm_s_pytorch.py")),
                    reason="reference checkout not present (it is absent on the GPU box by design)")
def test_launcher_swaps_the_hot_path_under_the_unmodified_reference_run(tmp_path):
    """python -m dlrm_amd.launch: the reference's own run() builds OUR DLRM_Net from its CLI (construction only here —
    zero epochs — because the product path has no CPU fallback); with one epoch it must fail loudly, not fall back."""
    import subprocess
    import sys
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1")
    probe = ("import sys, numpy as np; sys.argv=['x']; from dlrm_amd import launch; import dlrm_amd; "
             "ref = launch.load_reference(%r); assert ref.DLRM_Net is dlrm_amd.DLRM_Net; "
             "assert ref.ext_dist is dlrm_amd.ext_dist; print('swapped')" % REFERENCE)
    r = subprocess.run([sys.executable, "-c", probe], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "swapped" in r.stdout, r.stderr[-2000:]
    cli = ["--arch-sparse-feature-size=16", "--arch-embedding-size=1000-1000-1000", "--arch-mlp-bot=13-512-16",
           "--arch-mlp-top=22-256-1", "--mini-batch-size=128", "--data-generation=random", "--num-batches=2"]
    base = [sys.executable, "-m", "dlrm_amd.launch", "--reference", REFERENCE, "--"]
    r = subprocess.run(base + cli + ["--nepochs=0"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run(base + cli + ["--nepochs=1"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "no CPU fallback" in r.stderr


def test_embedding_update_plan_for_sgd_and_rowwise_adagrad():
    """The optimizer-step pre-hook's plan: SGD -> ("sgd", lr); RWSAdagrad (ours, and the reference's own class when the
    reference checkout is present) -> clr = lr / (1 + (step-1)*lr_decay) (optim/rwsadagrad.py:113-115), row-wise state
    created lazily in optimizer.state[p]["momentum"] with initial_accumulator_value, step counted per table."""
    import sys
    from dlrm_amd.dlrm_net import _embedding_update_plan
    from dlrm_amd.optim import FusedRWSAdagrad
    tables = [torch.nn.Parameter(torch.zeros(7, 4)), torch.nn.Parameter(torch.zeros(3, 4))]
    dense = torch.nn.Parameter(torch.zeros(5))
    sgd = torch.optim.SGD(tables + [dense], lr=0.25)
    assert _embedding_update_plan(sgd, tables) == ("sgd", 0.25)
    assert _embedding_update_plan(torch.optim.SGD([dense], lr=0.1), tables) is None      # does not own the tables
    # optimizers the fused kernels do not implement take the reference's own route: the sparse COO gradient is
    # materialised (dlrm_emb_bwd_coo) and the optimizer's step consumes it
    assert _embedding_update_plan(torch.optim.SGD(tables, lr=0.1, momentum=0.9), tables) == ("coo",)
    assert _embedding_update_plan(torch.optim.Adagrad(tables, lr=0.1), tables) == ("coo",)
    with pytest.raises(SystemExit):          # gradient accumulation + the non-linear fused row-wise update: refused, not approximated
        _embedding_update_plan(FusedRWSAdagrad(tables, lr=0.1), tables, count=2)
    classes = [FusedRWSAdagrad]
    if os.path.isfile(os.path.join(REFERENCE, "optim", "rwsadagrad.py")):
        sys.path.insert(0, os.path.join(REFERENCE, "optim"))
        import rwsadagrad
        classes.append(rwsadagrad.RWSAdagrad)
    for cls in classes:
        opt = cls(tables + [dense], lr=0.5, lr_decay=0.1, initial_accumulator_value=0.25, eps=1e-7)
        kind, clr, eps, states = _embedding_update_plan(opt, tables)
        assert kind == "rwsadagrad" and clr == 0.5 and eps == 1e-7
        assert [tuple(s_.shape) for s_ in states] == [(7,), (3,)] and all(float(s_[0]) == 0.25 for s_ in states)
        assert states[0] is opt.state[tables[0]]["momentum"] and opt.state[tables[1]]["step"] == 1
        _, clr2, _, states2 = _embedding_update_plan(opt, tables)
        assert abs(clr2 - 0.5 / 1.1) < 1e-12 and states2[0] is states[0] and opt.state[tables[0]]["step"] == 2


def test_accumulation_guard_compares_tables_not_argument_tuples():
    """every forward call hands EmbeddingBagsFunction a FRESH tuple of the same tables, so two parked backward
    passes must be recognised by table identity; with tuple identity the guard of the non-linear row-wise update never fired."""
    import dlrm_amd
    from dlrm_amd.optim import FusedRWSAdagrad
    tables = [torch.nn.Parameter(torch.zeros(7, 4)), torch.nn.Parameter(torch.zeros(3, 4))]
    opt = FusedRWSAdagrad(tables, lr=0.1)
    shell = dlrm_amd.DLRM_Net()
    pending = [(tuple(tables), None, None), (tuple(tables), None, None)]        # two distinct tuples, same tables
    assert pending[0][0] is not pending[1][0]
    with pytest.raises(SystemExit) as e:
        shell._apply_pending(pending, opt, None)
    assert "gradient accumulation" in str(e.value)
    assert opt.state[tables[0]].get("step", 0) == 0                             # refused before any state was advanced
    # tables of ANOTHER model parked beside them do not count
    other = [torch.nn.Parameter(torch.zeros(5, 4))]
    opt2 = FusedRWSAdagrad(tables + other, lr=0.1)
    from dlrm_amd.dlrm_net import _embedding_update_plan
    key = tuple(id(w) for w in tables)
    assert sum(1 for p_ in [(tuple(tables),), (tuple(other),)] if tuple(id(w) for w in p_[0]) == key) == 1
    assert _embedding_update_plan(opt2, tables, count=1)[0] == "rwsadagrad"


def test_flat_gradient_slots_live_on_the_parameter_and_die_with_the_wrapper():
    """the flat-buffer slot of a FlatDDP-wrapped parameter is an attribute of the Parameter (validated at use), not an
    entry of a process-global table keyed by its address; releasing / collecting the wrapper removes it."""
    import gc
    from dlrm_amd import ext_dist, functional
    tower = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.ReLU())
    w = ext_dist.FlatDDP(tower, broadcast=False)
    p = tower[0].weight
    v = functional._grad_out(p)
    assert v.data_ptr() == w.flat.data_ptr() and v.shape == p.shape
    functional.ARENA_BUSY.clear()
    assert not hasattr(functional, "GRAD_ARENAS")
    p._dlrm_grad_arena = (p._dlrm_grad_arena[0], 10 ** 6)                       # a slot that no longer fits is an error, not a stray write
    with pytest.raises(RuntimeError):
        functional._grad_out(p)
    del w
    gc.collect()
    assert not hasattr(p, "_dlrm_grad_arena")
    assert functional._grad_out(p).data_ptr() != 0 and not functional.ARENA_BUSY


def test_oracle_ref_recipe_builds_an_importable_sourceless_reference(tmp_path):
    """`make -C oracle ref` (oracle/build_ref.py): the reference's modules compiled where they lie into oracle/_ref/*.pyc — no
    source text in the tree — import and run on a box without a checkout (here: a subprocess that cannot see /root/reference)."""
    import subprocess
    import sys
    from oracle import build_ref
    if os.path.isfile(os.path.join(REFERENCE, "dlrm_s_pytorch.py")):
        assert build_ref.build(REFERENCE, quiet=True) == build_ref.OUT
    d = build_ref.ref_dir()
    if d is None:
        pytest.skip("no reference checkout and no prebuilt oracle/_ref")
    assert not [f for _, _, fs in os.walk(d) for f in fs if f.endswith(".py")], "reference SOURCES must never be copied"
    manifest = json.load(open(os.path.join(d, "MANIFEST.json")))
    assert set(manifest["modules"]) >= {"dlrm_s_pytorch.py", "extend_distributed.py", "optim/rwsadagrad.py"}
    probe = ("import sys, types; tb = types.ModuleType('torch.utils.tensorboard'); tb.SummaryWriter = object; import torch.utils; "
             "sys.modules['torch.utils.tensorboard'] = tb; sys.path[:] = [p for p in sys.path if 'reference' not in p]; "
             "sys.path.insert(0, %r); import dlrm_s_pytorch as r, optim.rwsadagrad as o; "
             "assert r.__file__.endswith('.pyc') and hasattr(r, 'DLRM_Net') and hasattr(o, 'RWSAdagrad'); print('ok')" % d)
    r = subprocess.run([sys.executable, "-c", probe], cwd=tmp_path, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
    # the launcher accepts the compiled tree as --reference
    base = [sys.executable, "-m", "dlrm_amd.launch", "--reference", d, "--", "--arch-sparse-feature-size=16",
            "--arch-embedding-size=100-100", "--arch-mlp-bot=13-32-16", "--arch-mlp-top=19-8-1", "--mini-batch-size=16",
            "--data-generation=random", "--num-batches=2", "--nepochs=0"]
    r = subprocess.run(base, cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_fused_rwsadagrad_hyperparameter_checks():
    from dlrm_amd.optim import FusedRWSAdagrad
    p = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (dict(lr=-1.0), dict(lr_decay=-0.1), dict(eps=-1e-3), dict(initial_accumulator_value=-1.0), dict(weight_decay=0.1)):
        with pytest.raises(ValueError):
            FusedRWSAdagrad(p, **bad)
    opt = FusedRWSAdagrad(p, lr=0.1)
    assert opt.state[p[0]]["step"] == 0 and opt.defaults["eps"] == 1e-10 and opt.defaults["lr_decay"] == 0.0


def test_graph_input_helpers():
    """Static-input bookkeeping of the whole-step HIP graph: shared tensors stay shared, stale shapes are refused."""
    from dlrm_amd.graph import _clone_struct, _copy_struct
    off = torch.arange(5)
    lst = [off, off, torch.arange(5) * 2]
    st = _clone_struct(lst)
    assert st[0] is st[1] and st[0] is not off and torch.equal(st[2], lst[2])
    _copy_struct(st, [off + 1, off + 1, off * 3])
    assert torch.equal(st[0], off + 1) and torch.equal(st[2], off * 3)
    t = _clone_struct(torch.ones(2, 3))
    _copy_struct(t, torch.zeros(2, 3))
    assert float(t.sum()) == 0
    with pytest.raises(RuntimeError, match="shape"):
        _copy_struct(t, torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="shape"):
        _copy_struct(st, [off, off, torch.arange(6)])
    with pytest.raises(RuntimeError, match="structure"):
        _copy_struct(st, [off, off])


def test_graph_input_pairs_for_the_raw_replay():
    """The raw replay path (dlrm_graph_replay: wait + input copies + hipGraphLaunch in one C call) takes its (static, caller) segments from
    a StagePlan, behind the same checks as the copy_ path: one segment per DISTINCT static tensor, source == destination (which the C side
    skips) where the caller already passed the static buffer, the shape / structure errors unchanged."""
    from dlrm_amd.graph import StagePlan, _check_struct, _clone_struct
    off = torch.arange(5)
    st = _clone_struct([off, off, torch.arange(5) * 2])
    a, b = off + 1, off * 3
    plan = StagePlan((st,), ([a, a, b],))
    plan.patch(([a, a, b],))
    assert plan.n == 2 and [plan.dst[j] for j in range(2)] == [st[0].data_ptr(), st[2].data_ptr()]
    assert [plan.src[j] for j in range(2)] == [a.data_ptr(), b.data_ptr()] and [plan.nbytes[j] for j in range(2)] == [40, 40]
    assert torch.equal(st[0], off)                      # nothing was copied: the segments are for the C call
    plan.patch(([st[0], st[1], b],))                    # the caller handed the static buffers back: only the third tensor moves
    assert plan.src[0] == plan.dst[0] and plan.src[1] == b.data_ptr() != plan.dst[1]
    with pytest.raises(RuntimeError, match="shape"):
        _check_struct(st, [a, a, torch.arange(6)])
    with pytest.raises(RuntimeError, match="structure"):
        _check_struct(st, [a, a])
    t = _clone_struct(torch.ones(2, 3))
    plan = StagePlan((t,), (t,))
    plan.patch((t,))
    assert plan.n == 1 and plan.src[0] == plan.dst[0] and plan.nbytes[0] == 24


def test_step_shaped_stage_plan_and_its_device_predicate():
    """The plan GraphedTrainStep builds over (X, offsets, indices, T): one segment for each tensor, one for an offsets tensor the tables
    share; takes() — the raw path's condition — is false for a tensor on another device and for a strided view.  (Once with
    the static buffers on the meta device: a device that a host tensor is foreign to, without a GPU.)"""
    from dlrm_amd.graph import StagePlan, _clone_struct
    B, T = 6, 3

    def request(dev):
        off = torch.arange(B, device=dev)
        return (torch.zeros(B, 13, device=dev), [off] * T, [torch.zeros(B, dtype=torch.int64, device=dev) for _ in range(T)],
                torch.zeros(B, 1, device=dev))
    for here, elsewhere in (("cpu", "meta"), ("meta", "cpu")):     # (real pointers; then static buffers a host tensor is foreign to)
        X, lS_o, lS_i, Y = like = request(here)
        static = (X.clone(), _clone_struct(lS_o), _clone_struct(lS_i), Y.clone())
        plan = StagePlan(static, like)
        assert plan.n == 1 + 1 + T + 1 and plan.flat
        assert plan.entries == [(0, None, None), (1, 0, None)] + [(2, k, None) for k in range(T)] + [(3, None, None)]
        assert plan.cap == [B * 13 * 4, B * 8] + [B * 8] * T + [B * 4]
        want = [static[0], static[1][0]] + static[2] + [static[3]]
        assert [plan.dst[j] or 0 for j in range(plan.n)] == [t.data_ptr() for t in want]
        assert here == "meta" or len(set(plan.dst[j] for j in range(plan.n))) == plan.n
        assert plan.takes(like) and plan.takes(request(here))
        far = request(elsewhere)
        assert not plan.takes(far) and not plan.takes((X, lS_o, lS_i, far[3])) and not plan.takes((X, lS_o, lS_i[:2] + far[2][2:], Y))
        wide = torch.zeros(B, 26, device=here)
        assert not plan.takes((wide[:, ::2], lS_o, lS_i, Y)) and not plan.takes((wide[:, :13], lS_o, lS_i, Y))
    # on the host's own device, with real pointers: a static tensor that kept the strides of a permuted first input is no run of bytes
    Xt = torch.zeros(13, B).t()
    Y = torch.zeros(B, 1)
    permuted = StagePlan((Xt.clone(), Y.clone()), (Xt, Y))
    assert not permuted.flat and not permuted.takes((torch.zeros(B, 13), Y))


@pytest.mark.parametrize("export", ["dlrm_graph_replay", "dlrm_forward_replay@0", "dlrm_forward_replay@1000000"])
def test_replay_exports_refuse_bad_arguments_before_any_device_call(export):
    """Both replay calls are one implementation (csrc/replay.h): DLRM_E_ARG for n < 0, a null graph handle, null arrays with n > 0, and —
    with sync_first = 0 — for a segment without a destination, all before the first HIP call (this test has no GPU to call).  The
    forward's call on both sides of its memcpy threshold."""
    import ctypes as C
    from dlrm_amd import _lib
    lib, E_ARG = _lib.load(), -1
    name, _, threshold = export.partition("@")
    keep = torch.zeros(4)
    fake_exec, stream = C.c_void_p(keep.data_ptr()), C.c_void_p(0)       # (never dereferenced: every call returns before using it)

    def call(n, dst, src, nb, graph_exec):
        if name == "dlrm_graph_replay":
            return lib.dlrm_graph_replay(n, dst, src, nb, 0, None, None, graph_exec, 0, stream)
        return lib.dlrm_forward_replay(n, dst, src, nb, int(threshold), graph_exec, 0, stream)
    one = lambda v: (C.c_void_p * 1)(v)                 # noqa: E731
    dst, src, nb = one(keep.data_ptr()), one(keep.data_ptr()), (C.c_int64 * 1)(16)
    assert call(-1, dst, src, nb, fake_exec) == E_ARG
    assert call(1, dst, src, nb, None) == E_ARG and call(0, None, None, None, None) == E_ARG
    for arrays in ((None, src, nb), (dst, None, nb), (dst, src, None)):
        assert call(1, *arrays, fake_exec) == E_ARG
    assert call(1, one(None), src, nb, fake_exec) == E_ARG
    assert call(1, dst, one(None), nb, fake_exec) == E_ARG
    assert call(1, dst, src, (C.c_int64 * 1)(-4), fake_exec) == E_ARG


def test_small_batch_tower_path_is_chosen_by_rows_widths_and_weight_traffic(monkeypatch):
    """functional._tower_applies: the whole-tower kernels (csrc/tower.hip) take native-fp32 towers of small batches only — at most
    TOWER_ROWS rows, widths the kernels hold in LDS (<= 512), at most 8 layers, and (M / 16) x parameters x 4 bytes of weight streaming
    under TOWER_L2_BYTES: Criteo-Kaggle's towers at 2048 rows yes (bench/dlrm_s_criteo_kaggle.sh:24), the Criteo-Terabyte towers never
    (1024-wide layers), any tower at the headline batch no."""
    from dlrm_amd import functional, ops

    class T:                                             # the attributes _tower_applies reads of a tensor
        def __init__(self, *shape, cuda=True):
            self.shape, self.is_cuda = shape, cuda

        def size(self, i):
            return self.shape[i]

    def tower(widths):
        ps = []
        for k, n in zip(widths[:-1], widths[1:]):
            ps += [T(n, k), T(n)]
        return ps

    f32, bf16 = ops.arith_code("f32"), ops.arith_code("bf16")
    monkeypatch.setattr(functional, "TOWER_ROWS", 4096)
    monkeypatch.setattr(functional, "TOWER_L2_BYTES", 384 << 20)
    kag_bot, kag_top = [13, 512, 256, 64, 16], [367, 512, 256, 1]
    tb_bot, tb_top = [13, 512, 256, 128], [479, 1024, 1024, 512, 256, 1]
    ok = lambda M, w, xw=None, arith=f32, cuda=True: functional._tower_applies(T(M, xw or w[0], cuda=cuda), arith, tower(w), len(w) - 1)   # noqa: E731
    assert ok(2048, kag_bot) and ok(2048, kag_top, xw=368) and ok(128, kag_bot) and ok(1, [4, 4])
    assert not ok(2048, kag_top, xw=370)                 # an input that is neither the true nor the padded width
    assert not ok(2048, tb_top, xw=480)                  # 1024-wide layers do not fit the kernels' LDS buffers
    assert ok(2048, tb_bot) and not ok(8192, tb_bot)     # rows
    assert not ok(65536, kag_bot) and not ok(0, kag_bot)
    assert not ok(2048, kag_bot, arith=bf16) and not ok(2048, kag_bot, cuda=False)
    assert not ok(64, [16] * 10)                         # more layers than a launch takes
    wide = [512] * 9                                     # 8 layers of 512 x 512: 8 MB of weights per 16-row workgroup
    assert ok(256, wide) and not ok(4096, wide)          # 16 x 8 MB = 128 MB of streaming yes, 256 x 8 MB = 2 GB no
    monkeypatch.setattr(functional, "TOWER_ROWS", 0)
    assert not ok(2048, kag_bot)


def test_data_front_ends_refuse_cpu_and_malformed_input(tmp_path):
    from dlrm_amd.criteo_bin import CriteoBinBatches, batch_byte_range, num_batches
    from dlrm_amd.datagen import UniformBatchGenerator
    from dlrm_amd.evaluate import inference
    with pytest.raises(RuntimeError, match="GPU"):
        UniformBatchGenerator(13, [10, 20], device="cpu")
    g = object.__new__(UniformBatchGenerator)
    g.seed = 5
    seeds = {g._seed(b, s_) for b in range(50) for s_ in (1, 2, 16, 48)}
    assert len(seeds) == 200 and all(0 <= x < 2 ** 64 for x in seeds)
    bad = tmp_path / "bad.bin"
    bad.write_bytes(b"\0" * 161)
    with pytest.raises(RuntimeError, match="160-byte"):
        CriteoBinBatches(str(bad), 4)
    ok = tmp_path / "ok.bin"
    ok.write_bytes(b"\0" * 160 * 10)
    with pytest.raises(RuntimeError, match="GPU"):
        CriteoBinBatches(str(ok), 4, device="cpu")
    assert num_batches(1600, 4) == 3 and batch_byte_range(1600, 4, 2) == (1280, 1600)
    with pytest.raises(RuntimeError, match="no test batch"):
        inference(None, [])


def test_chunk_pack_permutation_and_gradient():
    """Row bookkeeping of the pipelined all-to-all (functional.ChunkPackFunction): chunk c holds, per destination rank r,
    rows r*Bl + c*Bc .. of the global batch; backward routes every gradient row back to its global position."""
    from dlrm_amd.functional import ChunkPackFunction
    N, C, Bc, W = 3, 4, 2, 5
    B = N * C * Bc
    E = torch.arange(B * W, dtype=torch.float32).view(B, W).requires_grad_()
    outs = ChunkPackFunction.apply(E, N, C)
    assert len(outs) == C and all(o.shape == (N * Bc, W) and o.is_contiguous() for o in outs)
    for c in range(C):
        for r in range(N):
            assert torch.equal(outs[c][r * Bc:(r + 1) * Bc], E.detach()[r * C * Bc + c * Bc:r * C * Bc + (c + 1) * Bc])
    sum((o * (i + 1)).sum() for i, o in enumerate(outs)).backward()
    want = torch.tensor([(b % (C * Bc)) // Bc + 1.0 for b in range(B)]).view(B, 1).expand(B, W)
    assert torch.equal(E.grad, want)
    with pytest.raises(RuntimeError, match="split"):
        ChunkPackFunction.apply(torch.zeros(10, 2), 3, 2)


def test_dense_sync_environment_switch_resolves_ddp_to_the_flat_wrapper():
    """DLRM_DENSE_SYNC=flat: the reference's run() calls ext_dist.DDP(tower, device_ids=[...]) and gets the flat-buffer wrapper
    (same constructor surface); unset, ext_dist.DDP is torch's DistributedDataParallel, re-exported as the reference does."""
    import subprocess
    import sys
    code = ("from dlrm_amd import ext_dist; import inspect; "
            "print(ext_dist.DDP.__name__, 'device_ids' in inspect.signature(ext_dist.FlatDDP.__init__).parameters, ext_dist.TorchDDP.__name__)")
    for env, want in (({"DLRM_DENSE_SYNC": "flat"}, "FlatDDP True DistributedDataParallel"), ({}, "DistributedDataParallel True DistributedDataParallel")):
        e = {k: v for k, v in os.environ.items() if k != "DLRM_DENSE_SYNC"}
        e.update(env)
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == want, (r.stdout, r.stderr[-500:])


def test_fused_lookup_defaults_and_pmc_categories(monkeypatch):
    """The fused lookup + interaction path is the product default (DLRM_FUSE_EMB_INTERACT=0 and bench.py --no-fuse turn it off), and the
    PMC folding tool books the <NI, true> instantiations of the LDS-DMA interaction kernels under emb_interact_*, never under interact_*."""
    import importlib
    import sys as _sys
    import numpy as _np
    import dlrm_amd
    ln = _np.asarray([10, 20])
    kw = dict(m_spa=4, ln_emb=ln, ln_bot=_np.asarray([3, 4]), ln_top=_np.asarray([4 + 3, 2, 1]), arch_interaction_op="dot")
    _np.random.seed(0)
    assert dlrm_amd.DLRM_Net(**kw).fuse_emb_interact is True
    monkeypatch.setenv("DLRM_FUSE_EMB_INTERACT", "0")
    assert dlrm_amd.DLRM_Net(**kw).fuse_emb_interact is False
    monkeypatch.delenv("DLRM_FUSE_EMB_INTERACT")

    tools = os.path.join(ROOT, "tools")
    _sys.path.insert(0, tools)
    try:
        p2j = importlib.import_module("pmc_to_json")
    finally:
        _sys.path.remove(tools)
    fused, plain = "interact_fwd_dma_kernel<14, true>", "interact_fwd_dma_kernel<14, false>"
    assert p2j.in_cat("emb_interact_fwd", p2j.CATS["emb_interact_fwd"], fused) and not p2j.in_cat("interact_fwd", p2j.CATS["interact_fwd"], fused)
    assert p2j.in_cat("interact_fwd", p2j.CATS["interact_fwd"], plain) and not p2j.in_cat("emb_interact_fwd", p2j.CATS["emb_interact_fwd"], plain)
    assert p2j.in_cat("interact_bwd", p2j.CATS["interact_bwd"], "interact_bwd_kernel<2>") and p2j.in_cat("emb_fwd", p2j.CATS["emb_fwd"], "emb_fwd_kernel<4, 32, 1, long long, 2>")

    monkeypatch.setattr(_sys, "argv", ["bench.py"])
    bench = importlib.import_module("bench")
    assert bench.parse().fuse is True
    monkeypatch.setattr(_sys, "argv", ["bench.py", "--no-fuse"])
    assert bench.parse().fuse is False


def test_bench_gpus_n_launches_n_ranks_or_refuses(monkeypatch):
    """VERDICT r3 missing-3: `python bench.py --gpus 8` (no launcher around it) must never print an `n_gpus: 1` line.  With WORLD_SIZE
    unset and N > 1 bench.py re-executes itself under torch.distributed.run with one rank per GPU (the reference's own launch
    pattern, README.md:345-346); DLRM_BENCH_NO_SELF_LAUNCH=1 makes it exit with the command line instead; a launcher whose
    WORLD_SIZE disagrees with --gpus is refused with exit code 2."""
    import importlib
    import sys as _sys
    import types
    bench = importlib.import_module("bench")
    ns = lambda n: types.SimpleNamespace(gpus=n)     # noqa: E731
    assert bench.resolve_world(ns(1), [], {}) == ("run", 1)
    assert bench.resolve_world(ns(1), ["--gpus", "1"], {"WORLD_SIZE": "1"}) == ("run", 1)
    assert bench.resolve_world(ns(8), ["--gpus", "8"], {"WORLD_SIZE": "8", "RANK": "3"}) == ("run", 8)
    what, cmd = bench.resolve_world(ns(8), ["--gpus", "8", "--steps", "7", "--warmup", "2"], {})
    assert what == "exec" and cmd[0] == _sys.executable and cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == ["--gpus", "8", "--steps", "7", "--warmup", "2"] and cmd[-7].endswith("bench.py")
    with pytest.raises(SystemExit) as e:
        bench.resolve_world(ns(4), ["--gpus", "4"], {"DLRM_BENCH_NO_SELF_LAUNCH": "1"})
    assert "torch.distributed.run" in str(e.value.code) and "--nproc-per-node=4" in str(e.value.code)
    for env in ({"WORLD_SIZE": "2"}, {"WORLD_SIZE": "1"}):
        with pytest.raises(SystemExit) as e:
            bench.resolve_world(ns(8), ["--gpus", "8"], env)
        assert e.value.code == 2
    # end to end without a GPU: the re-executed command line is what actually runs (a stub "python" records its argv)
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([_sys.executable, "-c",
                        "import sys, os; sys.argv = ['bench.py', '--gpus', '2', '--steps', '1']; os.environ.pop('WORLD_SIZE', None)\n"
                        "import bench\n"
                        "os.execv = lambda exe, argv: (print('EXEC', ' '.join(argv)), sys.exit(0))\n"
                        "bench.main()"], cwd=root, capture_output=True, text=True, timeout=300,
                       env={k: v for k, v in os.environ.items() if k != "WORLD_SIZE"})
    assert r.returncode == 0 and "EXEC" in r.stdout and "--nproc-per-node=2" in r.stdout and "n_gpus" not in r.stdout, (r.stdout, r.stderr[-2000:])


def test_product_library_has_no_work_skipping_switches():
    """DLRM_GEMM_DEBUG / DLRM_INTERACT_DEBUG / DLRM_SEG_DEBUG (timing-only bits that make kernels skip work) exist
    only in a tuning build (`make TUNING=1`): the shipped library does not contain their names, so it cannot read them.
    VERDICT r5 #6 (round 6): the same now holds for EVERY environment variable the library ever read — launch-plan and schedule knobs
    (DLRM_GEMM_TM, DLRM_WGRAD_WGS, DLRM_SORT, DLRM_BF16_PHASED, ...) fold to their defaults at compile time (csrc/common.h DLRM_TUNE_ENV): no
    string of the shipped binary starts with DLRM_, and no source calls getenv outside the DLRM_TUNING block of common.h ("no process-wide
    mutable state": behaviour travels with the arguments of the call)."""
    import re
    from dlrm_amd import _lib
    _lib.load()
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in (b"DLRM_GEMM_DEBUG", b"DLRM_INTERACT_DEBUG", b"DLRM_SEG_DEBUG"):
        assert name not in blob, name
    names = sorted(set(re.findall(rb"DLRM_[A-Z0-9_]{3,}", blob)))
    assert not names, "environment-style names in the product library: %r" % names
    for f in sorted(os.listdir(_lib.CSRC)):
        if f.endswith((".hip", ".h")):
            src = open(os.path.join(_lib.CSRC, f)).read()
            if f == "common.h":
                head, _, tail = src.partition("#ifdef DLRM_TUNING")
                body, _, rest = tail.partition("#else")
                assert "getenv" not in head and "getenv" not in rest, f
            else:
                assert "getenv" not in src, f
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "DLRM_TUNING" in mk and "TUNING" in mk


class _MLPTrace:
    """Recorder around the stand-ins of _mlp_standins: one line per call — the operator's name, every tensor argument as dtype, shape
    and an identity number (the order of the buffer's first appearance, so a wrong buffer shows up), every scalar argument, and what the
    call returned.  Every tensor seen stays alive until the trace is dropped: no address is handed out twice within a case."""

    def __init__(self):
        self.lines, self.calls, self._ids, self._keep = [], 0, {}, []

    def desc(self, v):
        if isinstance(v, torch.Tensor):
            key = (v.untyped_storage().data_ptr(), v.storage_offset(), tuple(v.shape), tuple(v.stride()), v.dtype)
            if key not in self._ids:
                self._ids[key] = len(self._ids)
                self._keep.append(v)
            return "%s[%s]#%d" % (str(v.dtype).replace("torch.", ""), "x".join(map(str, v.shape)), self._ids[key])
        if isinstance(v, (list, tuple)):
            return "(" + ", ".join(self.desc(e) for e in v) + ")"
        return str(v)

    def wrap(self, name, fn):
        def logged(*args, **kwargs):
            head = "%s(%s)" % (name, ", ".join([self.desc(a) for a in args] + ["%s=%s" % (k, self.desc(kwargs[k])) for k in sorted(kwargs)]))
            out = fn(*args, **kwargs)
            self.lines.append(head if out is None else head + " -> " + self.desc(out))
            self.calls += 1
            return out
        return logged

    def note(self, text):
        self.lines.append(text)

    def text(self):
        return "\n".join(self.lines) + "\n"


def _mlp_act(v, a):
    from dlrm_amd import ops
    return torch.relu(v) if a == ops.ACT_RELU else torch.sigmoid(v) if a == ops.ACT_SIGMOID else v


def _mlp_standins(monkeypatch, rec=None):
    """Every device operator MLPFunction calls, replaced by plain torch on the CPU; each asserts that the operands it is handed exist in
    the form it reads.  With `rec` (an _MLPTrace) every call — the allocations included — is also logged."""
    from dlrm_amd import functional, ops
    masks = {}
    act = _mlp_act

    def linear_fwd(X, W, b, a, Y, arith_, relu_bits=None):
        assert Y is not None and X is not None and X.dtype == torch.float32
        y = act(X[:, :W.size(1)] @ W.t() + (b if b is not None else 0), a)
        Y.copy_(y)
        if relu_bits is not None:
            masks[relu_bits.data_ptr()] = y > 0

    def act_bwd(dY, Y, a, dZ, db):
        dZ.copy_(dY * (Y > 0) if a == ops.ACT_RELU else dY * Y * (1 - Y) if a == ops.ACT_SIGMOID else dY)

    def linear_bwd_weight(dZ, X, dW, db, accumulate=False, arith=None, **_):
        assert dZ is not None and X is not None
        dW.copy_((dZ.t() @ X)[:, :dW.size(1)])
        if db is not None:
            db.copy_(dZ.sum(0))

    def linear_bwd_data(dZ, W, Xprev, mask_act, dprev, arith_, relu_bits=None):
        assert dZ is not None
        d = dZ @ W
        if mask_act == ops.ACT_RELU:
            d = d * (masks[relu_bits.data_ptr()] if relu_bits is not None else (Xprev > 0))
        dprev.copy_(d[:, :dprev.size(1)])

    def reduced(shape3):                       # stand-in for a reduced-width tensor: right shape / dtype, the fp32 values ride along
        return torch.zeros(shape3, dtype=torch.bfloat16)

    def cast_like(planes):
        def cast(src, Npad=None, category=None):
            M, N = src.shape
            Npad = Npad or N
            t = reduced((3, M, Npad) if planes else (M, Npad))
            t.f32 = torch.zeros((M, Npad)); t.f32[:, :N] = src
            return t
        return cast

    def cast_t_like(planes):
        return lambda src, Rpad=None, category=None: cast_like(planes)(src.t().contiguous(), Rpad)

    def gemm_like(planes):
        def gemm(A, Bm, bias, a, Cf, Cr, relu_bits_out=None, relu_bits_in=None, category=None, **_):
            assert A.dim() == (3 if planes else 2) and Bm.dim() == A.dim() and A.size(-1) == Bm.size(-1), (A.shape, Bm.shape)
            if planes:
                assert ops.gemm_bf16x6_ok(A.size(1), Bm.size(1), A.size(2)), (A.shape, Bm.shape)      # no other kernel reads planes
            y = act(A.f32 @ Bm.f32.t() + (bias if bias is not None else 0), a)
            if relu_bits_out is not None:
                masks[relu_bits_out.data_ptr()] = y > 0
            if relu_bits_in is not None:
                y = y * masks[relu_bits_in.data_ptr()]
            assert Cf is not None or Cr is not None
            if Cf is not None:
                Cf.copy_(y[:, :Cf.size(1)])
            if Cr is not None:
                assert tuple(Cr.shape[-2:]) == (A.size(-2), Bm.size(-2))
                Cr.f32 = y
        return gemm

    def wgrad_like(dZr, Xr, dW, db, accumulate=False):
        assert dZr.size(-2) == Xr.size(-2)
        dW.copy_((dZr.f32.t() @ Xr.f32)[:, :dW.size(1)])
        if db is not None:
            db.copy_(dZr.f32.sum(0))

    def pad_cols(src, Kp):
        t = torch.zeros((src.size(0), Kp)); t[:, :src.size(1)] = src
        return t

    def linear_head_bwd(dY, Y, a, X, W, xact_kind, dX, dW, db, accumulate=False):      # the N == 1 head in one pass: always takes it
        dz = torch.empty_like(dY)
        act_bwd(dY, Y, a, dz, None)
        linear_bwd_weight(dz, X, dW, db)
        linear_bwd_data(dz, W, X, xact_kind, dX, None)
        return True

    for name, fn in (("linear_fwd", linear_fwd), ("act_bwd", act_bwd), ("linear_bwd_weight", linear_bwd_weight), ("linear_bwd_data", linear_bwd_data),
                     ("linear_head_bwd", linear_head_bwd), ("pad_cols", pad_cols)):
        monkeypatch.setattr(ops, name, fn)
    def cast_multi_like(items, category=None):           # (round 5: all weight copies of a bf16 tower in one launch)
        return [(cast_like(False)(s_, cp) if cp else None, cast_t_like(False)(s_, rp) if rp else None) for s_, cp, rp in items]
    monkeypatch.setattr(functional._Bf16Store, "cast_multi", staticmethod(cast_multi_like))
    for store, planes in ((functional._PlaneStore, True), (functional._Bf16Store, False)):
        monkeypatch.setattr(store, "cast", staticmethod(cast_like(planes)))
        monkeypatch.setattr(store, "cast_t", staticmethod(cast_t_like(planes)))
        monkeypatch.setattr(store, "gemm", staticmethod(gemm_like(planes)))
        monkeypatch.setattr(store, "wgrad", staticmethod(wgrad_like))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: None)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    if rec is not None:
        for owner, names in ((ops, ("linear_fwd", "act_bwd", "linear_bwd_weight", "linear_bwd_data", "linear_head_bwd", "pad_cols", "relu_bits_alloc")),
                             (functional, ("alloc2d",)),
                             (functional._Bf16Store, ("cast", "cast_t", "cast_multi", "gemm", "wgrad", "empty")),
                             (functional._PlaneStore, ("cast", "cast_t", "gemm", "wgrad", "empty"))):
            for n in names:
                label = n if owner in (ops, functional) else "%s.%s" % (owner.__name__, n)
                fn = rec.wrap(label, getattr(owner, n))
                monkeypatch.setattr(owner, n, fn if owner in (ops, functional) else staticmethod(fn))


def _mlp_tower(ln, B, requires_grad=True):
    """seeded parameters, activations, input and incoming gradient of the tower ln[0] -> ... -> ln[-1] at B rows"""
    from dlrm_amd import ops
    rng = np.random.default_rng(0)
    L = len(ln) - 1
    params = []
    for i in range(L):
        params += [torch.tensor((rng.standard_normal((ln[i + 1], ln[i])) * np.sqrt(2 / (ln[i] + ln[i + 1]))).astype(np.float32), requires_grad=True),
                   torch.tensor((rng.standard_normal(ln[i + 1]) * 0.1).astype(np.float32), requires_grad=True)]
    acts = tuple([ops.ACT_RELU] * (L - 1) + [ops.ACT_SIGMOID if ln[-1] == 1 else ops.ACT_RELU])
    x = torch.tensor(rng.random((B, ln[0])).astype(np.float32), requires_grad=requires_grad)
    dy = torch.tensor(rng.standard_normal((B, ln[-1])).astype(np.float32))
    return params, acts, x, dy


@pytest.mark.parametrize("ln,B,arith", [([13, 512, 256, 128], 4096, "bf16x6"), ([479, 1024, 1024, 512, 256, 1], 4096, "bf16x6"),
                                        ([480, 1024, 512, 256], 2048, "bf16x6"), ([96, 64, 32], 512, "bf16x6"), ([256, 320, 192, 64], 1000, "bf16x6"),
                                        ([13, 512, 256, 128], 4096, "bf16"), ([479, 1024, 1024, 512, 256, 1], 4096, "bf16")])
def test_mlp_storage_plan_hands_every_consumer_what_it_reads(monkeypatch, ln, B, arith):
    """MLPFunction's storage plan (functional.py: which layer keeps fp32, which keeps only the reduced-width copy — bf16, or the three planes
    of arith "bf16x6" — and which kernel form every forward / data-gradient / weight-gradient product takes) with the device operators
    replaced by plain torch on the CPU: every operator asserts that the operands it is handed exist in the form it reads, and the tower's
    output and all gradients must equal torch autograd's.  The kernels themselves are tested on the GPU; this is the HOST logic around
    them — the towers of the Terabyte model (13 -> 16 padded first layer, a 128-wide and a 1-wide layer between reduced-width layers), a
    tower the planes kernel refuses entirely, and a batch that is not a multiple of 64 (fp32 weight gradients beside planes)."""
    from dlrm_amd import ops
    from dlrm_amd.functional import MLPFunction
    _mlp_standins(monkeypatch)
    act = _mlp_act
    L = len(ln) - 1
    params, acts, x, dy = _mlp_tower(ln, B)
    y = MLPFunction.apply(x, acts, None, ops.arith_code(arith), *params)
    y.backward(dy)
    got = [y.detach(), x.grad] + [p.grad for p in params]
    ps = [p.detach().clone().requires_grad_(True) for p in params]
    xr = x.detach().clone().requires_grad_(True)
    h = xr
    for i in range(L):
        h = act(h @ ps[2 * i].t() + ps[2 * i + 1], acts[i])
    h.backward(dy)
    ref = [h.detach(), xr.grad] + [p.grad for p in ps]
    for k, (a, b) in enumerate(zip(got, ref)):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=2e-3, atol=2e-3 * float(b.abs().max()), err_msg=str((ln, k)))


# ---- MLPFunction's call trace, case by case, against tests/fixtures/mlp_tower_trace.json -----------------------------------------------
# The fixture holds the SHA-256 and the call count of every case's trace AS RECORDED FROM THE COMMIT BEFORE the tower plan (_plan_tower)
# was introduced: `python tests/test_host_logic.py --record FILE` in a checkout of that commit with this file copied in.  It is never
# regenerated from newer code: a refactor of MLPFunction must reproduce it.
_TRACE_FIXTURE = os.path.join(ROOT, "tests", "fixtures", "mlp_tower_trace.json")
_TB_TOWERS = ([13, 512, 256, 128], [479, 1024, 1024, 512, 256, 1])
_TRACE_TOWERS = _TB_TOWERS + ([480, 1024, 512, 256], [96, 64, 32], [256, 320, 192, 64], [256, 200, 72, 64], [58, 128, 64], [256, 256])
_TRACE_SWITCHES = ("BF16_STORAGE", "BF16_LEAN", "MULTI_CAST", "RELU_BITS", "BF16X6_PLANES", "BF16_PHASED", "SMALL_BATCH_BITS")
_TRACE_ROWS = tuple(s + "=0" for s in _TRACE_SWITCHES) + ("x_without_grad", "no_grad", "out_slot_aligned", "out_slot_one_float_in",
                                                           "consumer_act_aligned", "consumer_act_unaligned", "head_accepts", "head_declines")


def _trace_cases():
    """default switches: towers x batches (256: the least the bf16 forms take; 300: no multiple of 64; 128: below 256) x arithmetic; then
    one thing changed at a time on the two Terabyte towers at 256 rows"""
    cases = [(ln, B, arith, None) for ln in _TRACE_TOWERS for B in (256, 300, 128) for arith in ("f32", "bf16", "bf16x6")]
    cases += [(ln, 256, arith, row) for ln in _TB_TOWERS for arith in ("f32", "bf16", "bf16x6") for row in _TRACE_ROWS]
    return cases


def _trace_id(case):
    ln, B, arith, row = case
    return "%s|%d|%s|%s" % ("-".join(map(str, ln)), B, arith, row or "default")


def _record_mlp_trace(monkeypatch, ln, B, arith, row):
    from dlrm_amd import functional, ops
    from dlrm_amd.functional import MLPFunction, OutSlot
    rec = _MLPTrace()
    _mlp_standins(monkeypatch, rec)
    if row is not None and row.endswith("=0"):
        name = row[:-2]
        if name == "SMALL_BATCH_BITS":
            monkeypatch.setattr(functional, name, 0)
        else:
            monkeypatch.setattr(ops if name == "BF16_PHASED" else functional, name, False)
    if row == "head_declines":
        monkeypatch.setattr(ops, "linear_head_bwd", rec.wrap("linear_head_bwd", lambda *a, **k: False))
    bwd = MLPFunction.backward

    def backward(ctx, dY):
        out = bwd(ctx, dY)
        rec.note("backward returns " + ", ".join("None" if g is None else "%s%s" % (rec.desc(g), tuple(g.stride())) for g in out))
        return out
    monkeypatch.setattr(MLPFunction, "backward", staticmethod(backward))

    params, acts, x, dy = _mlp_tower(ln, B, requires_grad=row != "x_without_grad")
    N = ln[-1]
    code = ops.arith_code(arith)
    slot = None
    if row in ("out_slot_aligned", "out_slot_one_float_in"):
        c0 = 0 if row == "out_slot_aligned" else 1
        slot = OutSlot(torch.zeros((B, 2 * functional._round4(N) + 4))[:, c0:c0 + N])
    if row in ("consumer_act_aligned", "consumer_act_unaligned"):
        code |= functional.MLP_CONSUMER_APPLIES_LAST_ACT
        c0 = 0 if row == "consumer_act_aligned" else 1
        wide = torch.zeros((B, 2 * functional._round4(N) + 4))
        wide[:, c0:c0 + N] = dy
        dy = wide[:, c0:c0 + N]
    for t in [x, dy] + params:
        rec.desc(t)                                                     # identity numbers of the inputs, in a fixed order
    try:
        if row == "no_grad":
            with torch.no_grad():
                y = MLPFunction.apply(x, acts, slot, code, *params)
        else:
            y = MLPFunction.apply(x, acts, slot, code, *params)
        saved = y.grad_fn.saved_tensors if y.grad_fn is not None else None
        rec.note("forward returns %s%s, saved %s" % (rec.desc(y), tuple(y.stride()), "nothing" if saved is None else rec.desc(saved)))
        if y.grad_fn is not None:
            y.backward(dy)
    except RuntimeError as e:
        rec.note("RuntimeError: %s" % e)
    return rec


@pytest.mark.parametrize("case", _trace_cases(), ids=_trace_id)
def test_mlp_call_trace_equals_the_recorded_one(monkeypatch, tmp_path, case):
    """Every operator call and allocation MLPFunction makes, forward and backward — names, shapes, dtypes, which buffer goes where, every
    scalar — equals, case by case, the trace recorded before the storage plan moved into _plan_tower (see _TRACE_FIXTURE above)."""
    want = json.load(open(_TRACE_FIXTURE))[_trace_id(case)]
    rec = _record_mlp_trace(monkeypatch, *case)
    import hashlib
    got = {"sha256": hashlib.sha256(rec.text().encode()).hexdigest(), "calls": rec.calls}
    if got != want:
        f = tmp_path / "trace.txt"
        f.write_text(rec.text())
        assert got == want, "the call trace of %s changed; the new one is in %s" % (_trace_id(case), f)


def test_tower_plan_hands_every_consumer_what_it_reads(monkeypatch):
    """functional._plan_tower with no tensor anywhere: at the workloads' real batches, on and off the GPU, every product of the plan finds
    its operands in the form it reads; the bf16 Terabyte towers keep fp32 after exactly the layers they kept before the plan was one
    object (read off the recorded traces at 256 rows: the bf16 plan depends on M only through M >= 256 and M % 64 == 0); and the
    whole-tower path is taken only on the GPU and within TOWER_ROWS / TOWER_L2_BYTES."""
    from dlrm_amd import functional, ops
    from dlrm_amd.functional import _plan_tower
    RELU, NONE = ops.ACT_RELU, ops.ACT_NONE
    monkeypatch.setattr(functional, "TOWER_ROWS", 4096)
    monkeypatch.setattr(functional, "TOWER_L2_BYTES", 384 << 20)

    def plan(ln, M, arith, gpu=True, need_grad=True, need_dx=True, in_width=None, **kw):
        L = len(ln) - 1
        acts = tuple([RELU] * (L - 1) + [ops.ACT_SIGMOID if ln[-1] == 1 else RELU])
        return _plan_tower(M, in_width or ln[0], [(ln[i + 1], ln[i]) for i in range(L)], acts, ops.arith_code(arith), need_grad,
                           need_grad and need_dx, gpu, **kw)

    def check(p, M, why):
        ls = p.layers
        L = len(ls)
        assert ls[-1].out32, why
        assert p.store is not None or not any(lp.fwd16 or lp.wgrad16 or lp.dgrad16 or lp.out16 or lp.dx16 for lp in ls), why
        for i, lp in enumerate(ls):
            below, above = (ls[i - 1] if i > 0 else None), (ls[i + 1] if i + 1 < L else None)
            in32 = below is None or below.out32                     # the layer's input exists as fp32 (the tower's input always does)
            dz32 = above is None or above.dx32                      # its incoming gradient exists as fp32 (the last layer's comes from act_bwd)
            dz_any = dz32 or above.dx16
            assert lp.out32 or lp.out16, (why, i)
            # forward: a reduced-width GEMM reads the reduced-width output below, or casts the fp32 one; an fp32 GEMM needs fp32
            assert (in32 or below.out16) if lp.fwd16 else in32, (why, i)
            assert not lp.out16 or (lp.fwd16 and above.fwd16 and above.kb == lp.N), (why, i)
            assert lp.bits == (above is not None and lp.act == RELU and p.need_bits), (why, i)
            if p.store is functional._PlaneStore:
                assert not lp.fwd16 or ops.gemm_bf16x6_ok(M, lp.N, lp.kb), (why, i)
                assert not lp.dgrad16 or ops.gemm_bf16x6_ok(M, lp.K, lp.N), (why, i)
            # weight gradient: reduced width from the kept reduced-width input and a gradient in either form; fp32 from fp32 operands
            assert (lp.fwd16 and dz_any and ops.linear_bwd_weight_bf16_shapes_ok(M, lp.N, lp.K)) if lp.wgrad16 else (in32 and dz32), (why, i)
            if not lp.need_dx:
                assert i == 0 and not p.need_dx, (why, i)
                continue
            assert lp.dx32 or lp.dx16, (why, i)
            assert lp.mask_act == (below.act if below is not None else NONE) and (not lp.mask_bits or below.bits), (why, i)
            if lp.dgrad16:
                assert dz_any and (lp.mask_act == NONE or (lp.mask_act == RELU and lp.mask_bits)), (why, i)
            else:
                assert dz32 and not lp.dx16 and lp.dx32, (why, i)
                assert lp.mask_act == NONE or in32, (why, i)           # ops.linear_bwd_data masks with the fp32 activation, bits or not
            if lp.mask_act not in (NONE, RELU):
                assert in32, (why, i)

    kag_bot, kag_top = [13, 512, 256, 64, 16], [367, 512, 256, 1]
    # (+ two towers in which a layer takes the reduced-width weight gradient but not the reduced-width data gradient — 200 and 72 are
    # multiples of 8, not of 32 — below a layer whose output the next GEMM reads as it is: the fp32 copy is kept for the mask alone)
    for ln in list(_TRACE_TOWERS) + [kag_bot, kag_top, [256, 256, 200, 64], [256, 128, 72, 64]]:
        for M in (65536, 2048):
            for arith in ("f32", "bf16", "bf16x6"):
                for gpu in (True, False):
                    for need_dx in (True, False):
                        for switch in (None, "BF16_LEAN", "RELU_BITS", "BF16_STORAGE", "BF16X6_PLANES"):
                            with monkeypatch.context() as mp:
                                if switch:
                                    mp.setattr(functional, switch, False)
                                p = plan(ln, M, arith, gpu=gpu, need_dx=need_dx)
                                assert not p.whole_tower or (gpu and arith == "f32" and M <= 4096), (ln, M, arith, gpu)
                                if not p.whole_tower:
                                    check(p, M, (ln, M, arith, gpu, need_dx, switch))
        p = plan(ln, 65536, "bf16", need_grad=False)                 # a forward that will not be differentiated plans no backward form
        assert not p.need_bits and not any(lp.bits or lp.wgrad16 or lp.wT16_multi for lp in p.layers)

    # the Terabyte towers, arith "bf16": fp32 is kept after the tower's output only (bottom), and after the 256-wide input of the
    # matrix-vector head and the head itself (top); every other activation is bf16 + sign bits
    for M in (65536, 2048):
        assert [lp.out32 for lp in plan(_TB_TOWERS[0], M, "bf16").layers] == [False, False, True]
        assert [lp.out32 for lp in plan(_TB_TOWERS[1], M, "bf16").layers] == [False, False, False, True, True]
        assert [lp.out32 for lp in plan(_TB_TOWERS[1], M, "bf16", in_width=480).layers] == [False, False, False, True, True]
    # first-layer width 58 -> 60: the plan asks for the padded width >= 64 and refuses, where the tensor-level check alone would round 58 up to 64
    p = plan([58, 128, 64], 65536, "bf16")
    assert p.Kp == 60 and p.pad_x and not p.layers[0].wgrad16 and p.layers[1].wgrad16

    # whole-tower kernels: Criteo-Kaggle's towers at 2048 rows on the GPU, never off it, never a tower with a 1024-wide layer, never the big batch
    for ln, w in ((kag_bot, None), (kag_top, 368)):
        p = plan(ln, 2048, "f32", in_width=w)
        assert p.whole_tower and p.store is None and all(lp.out32 for lp in p.layers) and not p.head_fused
        assert not plan(ln, 2048, "f32", gpu=False, in_width=w).whole_tower and not plan(ln, 65536, "f32", in_width=w).whole_tower
        assert not plan(ln, 2048, "bf16", in_width=w).whole_tower
    p = plan(kag_bot, 2048, "f32")
    assert (p.pad_x, p.Kp, p.layers[0].K, p.in_width) == (True, 16, 16, 13)       # per-layer forward GEMMs: the 13 columns are padded
    p = plan(kag_top, 2048, "f32", in_width=368)
    assert (p.pad_x, p.Kp, p.layers[0].K, p.in_width) == (False, 368, 368, 368)  # an input that arrives padded meets a padded weight
    assert not plan(_TB_TOWERS[1], 2048, "f32", in_width=480).whole_tower and plan(_TB_TOWERS[1], 2048, "f32", in_width=480).head_fused
    assert not plan(_TB_TOWERS[1], 2048, "f32", in_width=480, consumer_act=True).head_fused
    assert not plan([256, 1], 2048, "f32", gpu=False).head_fused              # a single layer has no layer below the head
    with monkeypatch.context() as mp:
        mp.setattr(functional, "TOWER_FWD", True)
        p = plan(kag_bot, 2048, "f32")
        assert p.whole_tower and p.tower_fwd and (p.pad_x, p.Kp, p.layers[0].K) == (False, 0, 13)
    with monkeypatch.context() as mp:
        mp.setattr(functional, "TOWER_L2_BYTES", 64 << 20)               # 128 workgroups x 0.6 MB of weights no longer fit
        assert not plan(kag_bot, 2048, "f32").whole_tower
    with monkeypatch.context() as mp:
        mp.setattr(functional, "TOWER_ROWS", 1024)
        assert not plan(kag_bot, 2048, "f32").whole_tower
    with pytest.raises(RuntimeError, match="MLP input width 14 does not match the first layer"):
        plan(kag_bot, 2048, "f32", in_width=14)


def test_bench_node_state_never_raises_and_reads_the_sysfs_format(tmp_path, monkeypatch):
    """bench.py's `box.node` diagnostics: on a machine without GPUs (here) it returns error notes instead of raising; the shader-clock parser
    reads the `pp_dpm_sclk` format the GPU boxes expose (captured in profiles/round4/visit_slow_box/sysfs_clocks.txt)."""
    import glob as _glob
    import bench
    out = bench.node_state()
    assert isinstance(out, dict)
    d = tmp_path / "card0" / "device"
    d.mkdir(parents=True)
    (d / "pp_dpm_sclk").write_text("0: 500Mhz\n1: 2393Mhz *\n2: 2400Mhz\n")
    d2 = tmp_path / "card8" / "device"
    d2.mkdir(parents=True)
    (d2 / "pp_dpm_sclk").write_text("S: 94Mhz *\n0: 500Mhz\n1: 2400Mhz\n")
    real = _glob.glob
    monkeypatch.setattr(_glob, "glob", lambda pat: sorted(real(str(tmp_path / "card*" / "device" / "pp_dpm_sclk"))) if "pp_dpm_sclk" in pat else real(pat))
    out = bench.node_state()
    assert out["sclk_mhz_all_cards"] == [2393, 94] and out["cards_at_high_clock"] == 1


def test_planes_kernel_preconditions_are_host_side():
    """dlrm_gemm_bf16x6_supported answers without touching a GPU (the host mirror asks it for every layer of every tower)."""
    from dlrm_amd import ops
    assert ops.round_x6_k(479) == 480 and ops.round_x6_k(16) == 16 and ops.round_x6_k(13) == 16
    assert ops.gemm_bf16x6_ok(65536, 1024, 480) and ops.gemm_bf16x6_ok(65536, 512, 16) and ops.gemm_bf16x6_ok(256, 192, 64)
    assert not ops.gemm_bf16x6_ok(65536, 128, 256)          # N < 192
    assert not ops.gemm_bf16x6_ok(128, 512, 256)            # M < 256
    assert not ops.gemm_bf16x6_ok(65536, 512, 24)           # K % 16
    assert not ops.gemm_bf16x6_ok(65536, 1, 256)


def test_bench_calibration_failures_do_not_cost_the_headline(monkeypatch, capsys):
    """measure_box_or_none swallows any probe failure (reported on stderr); merge_box tolerates a probe present on one side only."""
    import bench

    def boom(device, quick=False):
        raise RuntimeError("HIP out of memory")
    monkeypatch.setattr(bench, "measure_box", boom)
    assert bench.measure_box_or_none(torch.device("cpu")) is None
    assert "box calibration failed" in capsys.readouterr().err
    b0 = {"cu_count": 256, "mfma_f32_tflops": 156.0, "hbm_copy_gbps": 6200.0, "hbm_gather_gbps": 6100.0}
    b1 = {"cu_count": 256, "mfma_f32_tflops": 158.0, "hbm_copy_gbps": 6300.0, "hbm_gather_error": "OOM"}
    box = bench.merge_box(b0, b1)
    assert box["mfma_f32_tflops"] == 157.0 and box["hbm_copy_gbps"] == 6250.0 and box["hbm_gather_gbps"] == 6100.0
    assert box["hbm_gather_error"] == "OOM" and box["before"]["hbm_gather_gbps"] == 6100.0 and "hbm_gather_gbps" not in box["after"]


def test_bench_help_renders():
    """`python bench.py --help` (argparse expands %-formats in help strings: a bare "1.7 % (" in one of them made --help raise for two rounds)"""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--gpus" in r.stdout and "--mlp-arith" in r.stdout, r.stderr[-500:]


def test_bench_dump_outputs_files_dtypes_sample_and_limit(tmp_path, monkeypatch):
    """bench.py --dump-outputs (dump_outputs): loss + model output + every parameter as float32 .npy, small parameters whole, a large
    one as a fixed seeded row sample (an embedding table: plus the rows the last batch looked up) with its row numbers in float64; the
    same call gives the same files, shapes and row sets; more than the byte limit is an error, not a truncated dump."""
    import importlib
    import sys as _sys
    monkeypatch.setattr(_sys, "argv", ["bench.py"])
    bench = importlib.import_module("bench")

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            torch.manual_seed(0)
            self.emb_l = torch.nn.ModuleList([torch.nn.EmbeddingBag(bench.DUMP_FULL_ELEMS // 4 + 7, 8), torch.nn.EmbeddingBag(10, 8)])
            self.top_l = torch.nn.Linear(5, 1)

    net = Net()
    big_rows = net.emb_l[0].weight.size(0)
    idx = torch.tensor([[3, big_rows - 1, 3] + [5] * 300, [1, 2, 3] + [4] * 300])
    loss, Z = torch.tensor(0.25), torch.randn(6, 1)
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        bench.dump_outputs(str(d), loss, Z, net, idx)
    files = sorted(os.listdir(dirs[0]))
    assert files == sorted(os.listdir(dirs[1])) == sorted(
        ["loss.npy", "Z.npy", "emb_l.0.weight.sample.npy", "emb_l.0.weight.sampled_rows.npy", "emb_l.1.weight.npy",
         "top_l.weight.npy", "top_l.bias.npy"])
    got = {f: np.load(os.path.join(dirs[0], f)) for f in files}
    for f, a in got.items():
        assert a.dtype == (np.float64 if f.endswith(".sampled_rows.npy") else np.float32), f
        assert np.array_equal(a, np.load(os.path.join(dirs[1], f))), f
    assert got["loss.npy"].tolist() == [0.25] and np.array_equal(got["Z.npy"], Z.numpy())
    rows = got["emb_l.0.weight.sampled_rows.npy"].astype(np.int64)
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < big_rows
    assert {3, 5, big_rows - 1} <= set(rows.tolist()) and len(rows) <= bench.DUMP_SAMPLE_ROWS + bench.DUMP_LOOKED_UP_ROWS
    assert np.array_equal(got["emb_l.0.weight.sample.npy"], net.emb_l[0].weight.detach().numpy()[rows])
    assert np.array_equal(got["emb_l.1.weight.npy"], net.emb_l[1].weight.detach().numpy())
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1000)
    with pytest.raises(RuntimeError, match="exceed"):
        bench.dump_outputs(str(tmp_path / "c"), loss, Z, net, idx)
    assert not (tmp_path / "c").exists() or not os.listdir(tmp_path / "c")


class _StubEvent:
    def __init__(self):
        self.complete = False

    def query(self):
        return self.complete


class _StubPool:
    """what iota._drain reads of a flag pool: the host-visible verdict words"""

    def __init__(self):
        self.host = torch.zeros(4, dtype=torch.int32)
        self.dev = torch.zeros(4, dtype=torch.int32)


def test_producer_tag_names_object_version_and_address(monkeypatch):
    """The producer tag of the one-lookup-per-bag proof on CPU tensors (the logic needs no device): a tagged tensor is known to both
    proofs without a launch; a versioned in-place write voids the tag; copy.deepcopy carries the attribute but the copy is NOT tagged."""
    import copy
    from dlrm_amd import iota, ops
    monkeypatch.setattr(iota, "_iota_cache", {})
    t = ops.mark_one_lookup_per_bag(torch.arange(8))
    s0 = dict(ops.IOTA_STATS)
    assert iota._iota_tagged(t)
    assert ops.offsets_iota_state(t) is True and ops.offsets_are_iota_start([t, t]) is True and ops.offsets_are_iota(t) is True
    assert ops.IOTA_STATS["tagged"] == s0["tagged"] + 3
    assert {k: ops.IOTA_STATS[k] for k in s0 if k != "tagged"} == {k: s0[k] for k in s0 if k != "tagged"}
    dc = copy.deepcopy(t)
    assert getattr(dc, iota._IOTA_TAG, None) is not None and not iota._iota_tagged(dc) and iota._iota_tagged(t)
    assert not iota._iota_tagged(t.clone()) and getattr(t[:4], iota._IOTA_TAG, None) is None
    t[3] = 0
    assert not iota._iota_tagged(t)


def test_verdict_cache_is_per_object_and_version_and_evicts_dead_entries_first(monkeypatch):
    import weakref
    from dlrm_amd import iota, ops
    cache = {}
    monkeypatch.setattr(iota, "_iota_cache", cache)
    a, b = torch.arange(8), torch.arange(8)
    iota._iota_remember(a, True)
    iota._iota_remember(b, False)
    s0 = dict(ops.IOTA_STATS)
    assert iota._iota_cached(a) is True and iota._iota_cached(b) is False
    assert ops.offsets_iota_state(a) is True and ops.offsets_are_iota_start(b) is False and ops.offsets_iota_state([a, b]) is False
    assert ops.IOTA_STATS["cached"] == s0["cached"] + 3 and ops.IOTA_STATS["tagged"] == s0["tagged"]
    assert ops.offsets_iota_state([a, ops.mark_one_lookup_per_bag(torch.arange(8))]) is True        # tagged + cached: known, booked as cached
    assert ops.IOTA_STATS["cached"] == s0["cached"] + 4
    a[0] = 5                                                  # a versioned in-place write: the verdict is void
    assert iota._iota_cached(a) is None and iota._iota_cached(b) is False
    # a different object at a recycled id: the entry's weak reference names the OLD object
    c = torch.arange(8)
    cache[id(c)] = (weakref.ref(b), c._version, True)
    assert iota._iota_cached(c) is None
    cache[id(c)] = (lambda: None, c._version, True)           # ... or nothing any more
    assert iota._iota_cached(c) is None
    # eviction at > 256 entries: dead references go first, the live verdicts stay
    cache.clear()
    live = [torch.arange(2) for _ in range(200)]
    for t in live:
        iota._iota_remember(t, True)
    for _ in range(57):
        iota._iota_remember(torch.arange(2), False)           # (each dies at once; ids may repeat, so plant the entries by hand too)
    for k in range(57):
        cache[-1 - k] = (lambda: None, 0, False)
    assert len(cache) > 256
    iota._iota_remember(a, False)
    assert len(cache) == 201 and all(iota._iota_cached(t) is True for t in live) and iota._iota_cached(a) is False
    more = [torch.arange(2) for _ in range(56)]
    for t in more:
        iota._iota_remember(t, True)
    assert len(cache) == 257
    iota._iota_remember(b, True)                              # nothing dead to drop: the cache starts over
    assert len(cache) == 1 and iota._iota_cached(b) is True and iota._iota_cached(live[0]) is None


def test_pending_device_proofs_keep_their_pool_until_their_event_completes(monkeypatch):
    """dlrm_amd/iota.py, rules 1 and 2: an entry whose event is incomplete survives every drain and any number of newer entries, and
    holds its flag pool; only its weak references are forgotten beyond the bound.  A complete entry is resolved and dropped."""
    import gc
    import weakref
    from dlrm_amd import iota
    monkeypatch.setattr(iota, "_iota_cache", {})
    pending = []
    pool = _StubPool()
    pool_alive = weakref.ref(pool)
    t_old = torch.arange(8)
    old = iota._Pending(_StubEvent(), pool, 0, [weakref.ref(t_old)])
    pending.append(old)
    del pool
    for _ in range(5):
        iota._drain(pending)
    assert pending == [old] and old.refs and iota._iota_cached(t_old) is None
    newer_pool = _StubPool()
    newer_pool.host[2] = 3                                     # slot 2: three bags did not start at their own number
    tensors = [torch.arange(8) for _ in range(iota.PENDING_REMEMBERED + 6)]
    for k, t in enumerate(tensors):
        pending.append(iota._Pending(_StubEvent(), newer_pool, 1 + k % 2, [weakref.ref(t)]))
        iota._drain(pending)
    gc.collect()
    assert len(pending) == len(tensors) + 1 and pending[0] is old and pool_alive() is not None and pending[0].pool is pool_alive()
    assert not old.refs and not pending[6].refs and pending[7].refs and len(pending[-1].refs) == 1      # the bound forgets references, not entries
    # the old proof completes: nothing to remember any more (its references were forgotten), the entry and with it the pool go
    old.event.complete = True
    iota._drain(pending)
    del old
    gc.collect()
    assert len(pending) == len(tensors) and pool_alive() is None and iota._iota_cached(t_old) is None
    # the newest two complete: verdicts remembered for the tensors still alive; one whose tensor has died resolves without error
    pending[-1].event.complete = pending[-2].event.complete = pending[-3].event.complete = True
    slots = [pending[-3].slot, pending[-2].slot, pending[-1].slot]
    t_a, t_b = tensors[-2], tensors[-1]
    del tensors[-3:], t
    gc.collect()
    assert pending[-3].refs[0]() is None
    iota._drain(pending)
    assert len(pending) == iota.PENDING_REMEMBERED + 3
    assert iota._iota_cached(t_a) is (slots[1] != 2) and iota._iota_cached(t_b) is (slots[2] != 2) and slots[1] != slots[2]
    assert all(not p.event.query() for p in pending)


def test_scratch_cache_is_grow_only_per_kind_and_stream(monkeypatch):
    from dlrm_amd import ops
    monkeypatch.setattr(ops, "_scratch_ws", {})
    cpu = torch.device("cpu")
    e = ops._scratch("emb", 10, cpu, stream=1)
    assert e.dtype == torch.uint8 and e.numel() == 256                        # the sort workspace is at least 256 bytes
    assert ops._scratch("emb", 200, cpu, stream=1) is e and ops._scratch("emb", 0, cpu, stream=1) is e
    big = ops._scratch("emb", 1000, cpu, stream=1)
    assert big is not e and big.numel() == 1000 and ops._scratch("emb", 10, cpu, stream=1) is big       # grow-only: never shrinks
    assert ops._scratch("emb", 10, cpu, stream=2) is not big and ops._scratch("emb", 10, cpu, stream=2).numel() == 256
    assert ops._scratch("wgrad", 0, cpu, stream=1) is None and ops._scratch("wgrad", -1, cpu, stream=1) is None
    w = ops._scratch("wgrad", 10, cpu, stream=1)
    t = ops._scratch("tower", 10, cpu, stream=1)
    assert w.numel() == 10 and t.numel() == 10 and w is not t and ops._scratch("wgrad", 5, cpu, stream=1) is w
    assert ops._scratch("tower", 0, cpu, stream=3).numel() == 0
    assert set(ops._scratch_ws) == {("emb", cpu, 1), ("emb", cpu, 2), ("wgrad", cpu, 1), ("tower", cpu, 1), ("tower", cpu, 3)}
    assert [w_ for (_, d_, _), w_ in ops._scratch_ws.items() if d_ == cpu and w_ is big] == [big]     # what GraphedTrainStep pins


# ---- dlrm_net.fused_route against the table of routes as it stood before the selection became one function ----------------------------------
# kind -> (none_fused, host_proof, align at 8 bits / for unpacked rows, align at 4 bits, autograd); presort: "fp32" with update_in_backward only
_ROUTE_ROWS = {
    "narrow_quant": (True, False, 8, 4, False), "quant": (True, False, 8, 4, False),
    "narrow_qr": (False, True, 16, 16, True), "qr": (True, True, 16, 16, True),
    "narrow": (False, True, 16, 16, True), "fp32": (True, True, 16, 16, True),
    "narrow_bf16": (False, True, 8, 8, True), "bf16": (True, True, 16, 16, True),
}
_ROUTE_FLAGS = ("fuse_emb_interact", "fuse_quant_interact", "fuse_qr_interact", "fuse_bf16_interact", "fuse_narrow_interact")
_NARROW_MAXF, _WIDE_MAXF = 32, 27          # dlrm_interact_gather_narrow_ok: F <= GC_MAXF; dlrm_interact_gather_ok at D = 128: F <= 27


def _route_wanted(tables, F, D, bits, flags, uib=False, op="dot", gpu=True, pool=False, grad=False, bf16_rows=False):
    """the kind the table of routes names, or None"""
    if not (flags["fuse_emb_interact"] and op == "dot" and gpu) or tables == "md" or pool:
        return None
    narrow = flags["fuse_narrow_interact"] and D in (16, 32, 64) and F <= _NARROW_MAXF
    wide = D == 128 and F <= _WIDE_MAXF
    if tables == "quant":
        if not flags["fuse_quant_interact"] or grad:
            return None
        return "narrow_quant" if narrow else "quant" if wide else None
    if tables == "qr":
        if not flags["fuse_qr_interact"] or bf16_rows:
            return None
        return "narrow_qr" if narrow else "qr" if wide else None
    if tables == "bf16":
        if not flags["fuse_bf16_interact"]:
            return None
        return "narrow_bf16" if narrow else "bf16" if wide else None
    return "narrow" if narrow else "fp32" if wide else None


def test_fused_route_reproduces_the_table_of_routes():
    from dlrm_amd import ops
    from dlrm_amd.dlrm_net import FusedRoute, fused_route
    all_on = dict.fromkeys(_ROUTE_FLAGS, True)
    states = [all_on] + [dict(all_on, **{f: False}) for f in _ROUTE_FLAGS]
    others = [{}, {"uib": True}, {"op": "cat"}, {"gpu": False}, {"pool": True}, {"grad": True}, {"bf16_rows": True}]
    names = {"uib": "update_in_backward", "op": "interaction_op", "gpu": "on_gpu", "pool": "pooling_weights", "grad": "grad_wanted",
             "bf16_rows": "bf16_rows"}
    seen = set()
    for tables in ("fp32", "bf16", "qr", "md", "quant"):
        for D in (16, 32, 64, 128, 48):
            for F in (2, 27, 28, 33):
                for bits in ((4, 8) if tables == "quant" else (0,)):
                    for flags in states:
                        for other in others:
                            if other and flags is not all_on:
                                continue
                            why = (tables, D, F, bits, flags, other)
                            got = fused_route(tables, F, D, bits, **flags, **{"update_in_backward": False, **{names[k]: v for k, v in other.items()}})
                            kind = _route_wanted(tables, F, D, bits, flags, **other)
                            if kind is None:
                                assert got is None, why
                                continue
                            none_fused, host_proof, align8, align4, autograd = _ROUTE_ROWS[kind]
                            want = FusedRoute(kind, none_fused, host_proof, align4 if bits == 4 else align8,
                                              kind == "fp32" and bool(other.get("uib")), autograd)
                            assert got == want, why
                            seen.add(kind)
    assert seen == set(_ROUTE_ROWS) and set(_ROUTE_ROWS) == set(ops.ROW_KINDS) | {"fp32"}
    # a few rows of the table spelt out
    on = dict(all_on, update_in_backward=True)
    assert fused_route("fp32", 27, 128, **on) == FusedRoute("fp32", True, True, ops.GATHER_ALIGN, True, True)
    assert fused_route("fp32", 27, 16, **on) == FusedRoute("narrow", False, True, 16, False, True)
    assert fused_route("fp32", 27, 16, **dict(on, fuse_narrow_interact=False)) is None              # (the default model of the Kaggle step)
    assert fused_route("bf16", 27, 64, **on) == FusedRoute("narrow_bf16", False, True, 8, False, True)
    assert fused_route("qr", 4, 128, **on) == FusedRoute("qr", True, True, 16, False, True)
    assert fused_route("qr", 4, 128, bf16_rows=True, **on) is None and fused_route("md", 4, 16, **on) is None
    assert fused_route("quant", 27, 32, 4, **dict(on, update_in_backward=False)) == FusedRoute("narrow_quant", True, False, 4, False, False)
    assert fused_route("quant", 27, 128, 8, **dict(on, update_in_backward=False)) == FusedRoute("quant", True, False, 8, False, False)
    assert fused_route("quant", 27, 128, 8, grad_wanted=True, **on) is None
    assert isinstance(fused_route("fp32", 2, 128, **on), tuple)                                      # an immutable record
    with pytest.raises(AttributeError):
        fused_route("fp32", 2, 128, **on).kind = "qr"


def test_at_most_one_gather_ok_answers_for_a_table_kind_and_shape():
    """what one decision per (table kind, D, F) rests on: the D = 128 kernels and the narrow ones never both take a shape — and the limits
    _route_wanted states are the library's"""
    from dlrm_amd import ops
    pairs = {"fp32": (ops.gather_ok, ops.gather_narrow_ok), "bf16": (ops.gather_bf16_ok, ops.gather_narrow_bf16_ok),
             "qr": (ops.gather_qr_ok, ops.gather_narrow_qr_ok),
             "quant4": (lambda F, D: ops.gather_quant_ok(F, D, 4), lambda F, D: ops.gather_narrow_quant_ok(F, D, 4)),
             "quant8": (lambda F, D: ops.gather_quant_ok(F, D, 8), lambda F, D: ops.gather_narrow_quant_ok(F, D, 8))}
    for kind, (wide, narrow) in pairs.items():
        for D in (8, 16, 32, 48, 64, 96, 128, 256):
            for F in range(1, 40):
                w, n = wide(F, D), narrow(F, D)
                assert not (w and n), (kind, D, F)
                assert w == (D == 128 and F <= _WIDE_MAXF), (kind, D, F)
                assert n == (D in (16, 32, 64) and F <= _NARROW_MAXF), (kind, D, F)


# the seven refusals of the sparse embedding update, as the source held them (seven separate sys.exit blocks) before they became one table
_UPDATE_REFUSALS = {
    ("adagrad", "bf16"): "ERROR: the fused exact Adagrad update is not built for bfloat16 embedding tables; use SGD or row-wise Adagrad",
    ("adagrad", "qr"): "ERROR: the fused exact Adagrad update is not built for QR embedding tables; use SGD, or set "
                       "model.fused_emb_update = False (DLRM_FUSED_EMB_UPDATE=0) with a torch optimizer",
    ("adagrad", "md"): "ERROR: the fused exact Adagrad update is not built for mixed-dimension embedding tables; use SGD, or set "
                       "model.fused_emb_update = False (DLRM_FUSED_EMB_UPDATE=0) with a torch optimizer",
    ("rwsadagrad", "qr"): "ERROR: the fused row-wise Adagrad update is not built for QR embedding tables; use SGD, or set "
                          "model.fused_emb_update = False (DLRM_FUSED_EMB_UPDATE=0) with a torch optimizer",
    ("rwsadagrad", "md"): "ERROR: the fused row-wise Adagrad update is not built for mixed-dimension embedding tables; use SGD, or set "
                          "model.fused_emb_update = False (DLRM_FUSED_EMB_UPDATE=0) with a torch optimizer",
    ("coo", "bf16"): "ERROR: bfloat16 embedding tables are updated by the fused kernels only: plain SGD (no momentum, no weight "
                     "decay) or row-wise Adagrad; this optimizer needs the sparse COO gradient",
    ("unfused", "bf16"): "ERROR: bfloat16 embedding tables need the fused embedding update (fused_emb_update = False materialises sparse "
                         "fp32 COO gradients for a torch optimizer, which would round on every add)",
}


def test_update_refusal_table_answers_every_pair_with_the_recorded_strings():
    """(update kind, table kind) -> the exact message, or no refusal: every pair, through the one function that reads the table"""
    import dlrm_amd
    from dlrm_amd import dlrm_net
    assert dlrm_net.UPDATE_REFUSALS == _UPDATE_REFUSALS
    shell = dlrm_amd.DLRM_Net()
    for update in ("sgd", "rwsadagrad", "adagrad", "coo", "unfused"):
        for tables in ("fp32", "bf16", "qr", "md", "quant"):
            shell._table_kind = lambda tables=tables: tables
            want = _UPDATE_REFUSALS.get((update, tables))
            if want is None:
                shell._refuse_update(update)
            else:
                with pytest.raises(SystemExit) as e:
                    shell._refuse_update(update)
                assert e.value.code == want, (update, tables)


def test_table_kind_names_the_tables_the_refusals_are_keyed_by():
    import dlrm_amd
    np.random.seed(5)
    args = (np.asarray([300, 3, 40]), np.asarray([13, 8]), np.asarray([8 + 6, 1]), "dot")
    kw = dict(sigmoid_top=0, loss_function="bce")
    assert dlrm_amd.DLRM_Net(8, *args, **kw)._table_kind() == "fp32"
    assert dlrm_amd.DLRM_Net(8, *args, qr_flag=True, qr_operation="mult", qr_collisions=4, qr_threshold=200, **kw)._table_kind() == "qr"
    assert dlrm_amd.DLRM_Net([2, 8, 4], *args, md_flag=True, md_threshold=2, **kw)._table_kind() == "md"
    bf16 = dlrm_amd.DLRM_Net(8, *args, **kw)
    bf16.embedding_bfloat16("nearest")
    assert bf16._table_kind() == "bf16"


def test_parked_grad_accepts_the_three_and_the_four_element_form():
    from dlrm_amd.dlrm_net import ParkedGrad
    w, bags, dout, pre = (object(),), object(), object(), object()
    assert ParkedGrad(*(w, bags, dout)) == (w, bags, dout, None) and ParkedGrad(*(w, bags, dout)).presorted is None
    p = ParkedGrad(*(w, bags, dout, pre))
    assert (p.weights, p.bags, p.dout, p.presorted) == (w, bags, dout, pre) and len(p) == 4
    with pytest.raises(TypeError):
        ParkedGrad(*(w, bags))


if __name__ == "__main__":
    # python tests/test_host_logic.py --record FILE [--traces DIR]: write the fixture of test_mlp_call_trace_equals_the_recorded_one from
    # the dlrm_amd package of THIS checkout (and, with --traces, every case's full trace as text)
    import argparse
    import hashlib
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True)
    ap.add_argument("--traces")
    args = ap.parse_args()
    fixture = {}
    for case in _trace_cases():
        with pytest.MonkeyPatch.context() as mp:
            rec = _record_mlp_trace(mp, *case)
        fixture[_trace_id(case)] = {"sha256": hashlib.sha256(rec.text().encode()).hexdigest(), "calls": rec.calls}
        if args.traces:
            os.makedirs(args.traces, exist_ok=True)
            open(os.path.join(args.traces, _trace_id(case).replace("|", "_") + ".txt"), "w").write(rec.text())
    with open(args.record, "w") as f:
        json.dump(fixture, f, indent=0, sort_keys=True)
        f.write("\n")
