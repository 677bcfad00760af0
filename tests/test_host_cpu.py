"""CPU-side tests (no GPU): the C-ABI library loads and exports every symbol include/agan.h declares, the host mirror of
the reference interface has the reference's state_dict keys / parameter counts / initialisation, the product path refuses
to run without a GPU (no CPU fallback), and the data-parallel gradient exchange is exercised with gloo, world_size 2."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import GOLDEN, collect_from_children, free_port, load, sub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
agan = importlib.import_module("attention-gan_amd")
L = importlib.import_module("attention-gan_amd.backend.lib")
GEN = importlib.import_module("attention-gan_amd.networks.generator")
DISC = importlib.import_module("attention-gan_amd.networks.discriminators")
LAY = importlib.import_module("attention-gan_amd.utilities.layers")
OPT = importlib.import_module("attention-gan_amd.optim")
DP = importlib.import_module("attention-gan_amd.dataparallel")
TR = importlib.import_module("attention-gan_amd.trainers.trainer")


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "agan.h")).read()
    declared = set(re.findall(r"\b(agan_[a-z0-9_]+)\s*\(", header)) - {"agan_round_up"}
    lib = L.load()                       # dlopen + prototype attach raises if anything is missing
    assert lib.agan_version() == L.ABI_VERSION == 101
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(agan_[a-z0-9_]+)\b", out))
    assert declared <= exported, f"declared but not exported: {sorted(declared - exported)}"
    assert declared == set(L.EXPORTED_SYMBOLS), sorted(declared ^ set(L.EXPORTED_SYMBOLS))


def test_c_abi_argument_validation_without_gpu():
    """Entry points validate arguments before touching the device: bad geometry comes back as AGAN_EINVAL + message."""
    lib = L.load()
    g = L.ConvGeom()
    assert lib.agan_conv_gather_ws_bytes(g, L.PREC_F32) == 0
    assert lib.agan_packed_weight_bytes(L.PACK_UP_FWD, 8, 8, 4, 4, L.PREC_F32) == 0          # folded upsample conv is 3x3 only
    assert lib.agan_packed_weight_bytes(L.PACK_FWD, 3, 32, 3, 3, L.PREC_F32) == 32 * 9 * 32 * 4   # Nld = round_up(3, 32)
    assert lib.agan_packed_weight_bytes(L.PACK_UP_FWD, 64, 64, 3, 3, L.PREC_F32) == 4 * 64 * 4 * 64 * 4
    # 16-bit modes: [k-step = 16 channels of a tap][plane][Nld][16] x 2 bytes; 32 channels x 9 taps = 18 k-steps
    assert lib.agan_packed_weight_bytes(L.PACK_FWD, 3, 32, 3, 3, L.PREC_BF16X3) == 18 * 2 * 32 * 32
    assert lib.agan_packed_weight_bytes(L.PACK_FWD, 3, 32, 3, 3, L.PREC_BF16) == 18 * 1 * 32 * 32
    assert lib.agan_packed_weight_bytes(L.PACK_FWD, 3, 32, 3, 3, L.PREC_F16) == 18 * 1 * 32 * 32
    assert lib.agan_packed_weight_bytes(L.PACK_FWD, 3, 40, 4, 4, L.PREC_BF16X6) == 2 * 4 * 4 * 2 * 3 * 32 * 32   # 2 chunks x 4 phases x 4 taps
    assert lib.agan_packed_weight_bytes(L.PACK_FWD, 3, 32, 3, 3, L.PREC_F16X3) == 18 * 2 * 32 * 32  # fp16 hi/lo planes
    assert lib.agan_packed_weight_bytes(L.PACK_FWD, 3, 32, 3, 3, 9) == 0                           # unknown mode
    # effective precision: the patch kernels take 3x3 / 2x2-per-class / 4x4-s2 geometries with > 4 output channels
    g3 = L.ConvGeom()
    g3.B, g3.Cin, g3.IH, g3.IW, g3.Cout, g3.OH, g3.OW, g3.R, g3.S, g3.OS, g3.SY, g3.DY = 2, 16, 8, 8, 24, 8, 8, 3, 3, 1, 1, 1
    g3.OY[0] = g3.OY[1] = -1
    assert lib.agan_conv_effective_prec(g3, L.PREC_BF16) == L.PREC_BF16 and lib.agan_conv_effective_prec(g3, L.PREC_F32) == L.PREC_F32
    g3.Cout = 3
    assert lib.agan_conv_effective_prec(g3, L.PREC_BF16X6) == L.PREC_F32                         # RGB head: vector-ALU kernels
    g3.Cout, g3.R, g3.S, g3.OY[0], g3.OY[1] = 24, 1, 1, 0, 0
    assert lib.agan_conv_effective_prec(g3, L.PREC_F16) == L.PREC_F32                            # 1x1 / linear: fp32 MFMA
    rc = lib.agan_conv_gather(None, None, None, None, g, None, 0, 0, None, None, 0, None, None, None)
    assert rc == -1 and b"conv" in lib.agan_last_error()


def test_state_dict_keys_and_param_counts_match_reference():
    g = load("a5_generator")
    gf, emb, z, cond, _, _ = (int(v) for v in g["dims"])
    G = GEN.Generator(gf, emb, z, cond)
    assert set(G.state_dict()) == set(sub(g, "param/"))
    for k, v in sub(g, "param/").items():
        assert tuple(G.state_dict()[k].shape) == tuple(v.shape), k
    for res, cls in ((64, DISC.Disc64), (128, DISC.Disc128), (256, DISC.Disc256)):
        gd = load(f"a7_disc{res}")
        D = cls(int(gd["df"]))
        assert set(D.state_dict()) == set(sub(gd, "param/"))
    # parameter counts at the metric configuration (probed on the reference)
    count = lambda m: sum(p.numel() for p in m.parameters())
    assert count(GEN.Generator(32, 256, 100, 100)) == 7_084_592
    assert [count(c(64)) for c in (DISC.Disc64, DISC.Disc128, DISC.Disc256)] == [2_765_569, 15_875_841, 68_310_785]
    assert len(GEN.Generator(32, 256, 100, 100).state_dict()) == 97 and len(DISC.Disc256(64).state_dict()) == 45


def test_same_seed_gives_reference_initial_weights():
    """Module creation order and initialisers follow the reference, so torch.manual_seed(s) reproduces its init bit for bit
    (h1_init_seed7: the reference's Generator(4, 16, 10, 10) and Disc128(4) state_dicts after torch.manual_seed(7))."""
    ref = load("h1_init_seed7")
    torch.manual_seed(int(ref["seed"]))
    G, D = GEN.Generator(4, 16, 10, 10), DISC.Disc128(4)
    for name, mine in (("G", G), ("D", D)):
        want = sub(ref, name + "/")
        assert set(mine.state_dict()) == set(want), name
        for k, v in want.items():
            assert torch.equal(mine.state_dict()[k], v), f"{name}.{k}"


def test_no_cpu_fallback():
    G = GEN.Generator(4, 16, 10, 10)
    with pytest.raises(L.AganError, match="no CPU fallback"):
        G(torch.randn(2, 10), torch.randn(2, 16), torch.randn(2, 16, 5), torch.ones(2, 5, dtype=torch.int64), torch.randn(2, 10))
    with pytest.raises(L.AganError):
        DISC.Disc64(4)(torch.randn(2, 3, 64, 64))


def test_layers_factory_surface():
    assert LAY.Layers.calculate_out_hw(64, 4, 2, 1) == 32
    with pytest.raises(AssertionError, match="channels dont divide 2"):
        LAY.Layers.GLU()(torch.randn(1, 3, 2, 2))
    c = LAY.Layers.conv(8, 8, 16, 8)
    assert (c.kernel_size, c.stride, c.padding) == ((4, 4), (2, 2), (1, 1))
    assert set(LAY.Layers.upBlock(8, 4).state_dict()) == {"1.weight", "2.weight", "2.bias", "2.running_mean", "2.running_var", "2.num_batches_tracked"}
    with pytest.raises(Exception):
        LAY.Layers.conv(8, 8, 16, 1000)


def test_trainer_helpers():
    t = TR.ModelTrainer()
    m = t._make_mask(torch.tensor([3, 1, 2]))
    assert m.tolist() == [[1, 1, 1], [1, 0, 0], [1, 1, 0]] and m.dtype == torch.int64
    assert t._make_match_labels(4).tolist() == [0, 1, 2, 3]
    assert tuple(t._make_noise(3, 5).shape) == (3, 5)
    assert torch.allclose(t._denormalise_single(torch.tensor([-1.0, 1.0])), torch.tensor([0.0, 1.0]))


def test_flat_adam_rehomes_parameters_and_speaks_adam_state_dict():
    lin = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Linear(7, 3))
    before = {k: v.clone() for k, v in lin.state_dict().items()}
    opt = OPT.FlatAdam(lin.parameters(), lr=2e-4, betas=(0.5, 0.999))
    for k, v in lin.state_dict().items():
        assert torch.equal(v, before[k])
    base = opt.flat.data_ptr()
    for p, o in zip(opt.params, opt.offsets):
        assert p.data_ptr() == base + 4 * o and o % 4 == 0 and p.grad.data_ptr() == opt.grad.data_ptr() + 4 * o
    lin(torch.randn(2, 5)).sum().backward()
    assert float(opt.grad.abs().sum()) > 0                      # autograd accumulated straight into the flat buffer
    opt.zero_grad()                                             # no 4-byte-per-parameter fill: the first writer overwrites
    assert all(p.grad is None and not p._agan_grad_dst.written for p in opt.params)
    lin(torch.randn(2, 5)).sum().backward()
    assert opt._rebind() == len(opt.params) and float(opt.grad.abs().sum()) > 0   # stock torch grads are copied in
    opt.zero_grad()
    lin[0](torch.randn(2, 5)).sum().backward()                  # the second layer receives no gradient in this backward ...
    assert opt._rebind() == 2
    o2 = opt.offsets[2]
    assert float(opt.grad[o2:].abs().sum()) == 0 and float(opt.grad[:o2].abs().sum()) > 0    # ... so its slices are zeroed
    assert all(p.grad.data_ptr() == opt.grad.data_ptr() + 4 * o for p, o in zip(opt.params, opt.offsets))
    sd = opt.state_dict()
    ref = torch.optim.Adam(torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Linear(7, 3)).parameters(), lr=2e-4, betas=(0.5, 0.999))
    assert set(sd["param_groups"][0]) >= {"lr", "betas", "eps", "params"} and sd["param_groups"][0]["params"] == ref.state_dict()["param_groups"][0]["params"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()


def test_grad_bucket_partition():
    mods = torch.nn.Sequential(*[torch.nn.Linear(64, 64) for _ in range(6)])
    opt = OPT.FlatAdam(mods.parameters())
    bk = DP.GradBuckets(opt, bucket_bytes=2 * 64 * 64 * 4)
    assert bk.bounds[0][0] == 0 and bk.bounds[-1][1] == opt.numel
    assert all(a[1] == b[0] for a, b in zip(bk.bounds, bk.bounds[1:]))         # contiguous cover
    assert len(bk.bounds) >= 3 and sum(bk.counts) == len(opt.params)
    assert bk.finish() == 1.0


def _dp_worker(rank, world, port, q, bf16=False):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if bf16:
        os.environ["AGAN_DP_BF16"] = "1"
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.manual_seed(100 + rank)                                         # different init per rank on purpose
        net = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 8), torch.nn.Linear(8, 8))
        DP.broadcast_module_(net, 0)
        opt = OPT.FlatAdam(net.parameters())
        bk = DP.GradBuckets(opt, bucket_bytes=16 * 32 * 4)                    # several buckets
        x = torch.randn(4, 16, generator=torch.Generator().manual_seed(rank))
        opt.zero_grad()
        bk.arm()
        net(x).pow(2).sum().backward()
        local = None
        scale = bk.finish()
        q.put((rank, scale, opt.flat.clone(), opt.grad.clone(), len(bk.bounds)))
    finally:
        dist.destroy_process_group()


def test_data_parallel_gradient_exchange_gloo_world2():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(collect_from_children(q, procs, timeout=120), key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (r0, s0, w0, g0, nb0), (r1, s1, w1, g1, nb1) = got
    assert s0 == s1 == 0.5 and nb0 == nb1 and nb0 > 1
    assert torch.equal(w0, w1)                                   # broadcast made the replicas identical
    assert torch.equal(g0, g1)                                   # both hold the SUM of the two shards' gradients
    # single-process check: sum of per-shard gradients on the same weights
    net = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 8), torch.nn.Linear(8, 8))
    opt = OPT.FlatAdam(net.parameters())
    with torch.no_grad():
        opt.flat.copy_(w0)
    total = torch.zeros_like(opt.grad)
    for r in range(2):
        opt.zero_grad()
        net(torch.randn(4, 16, generator=torch.Generator().manual_seed(r))).pow(2).sum().backward()
        opt._rebind()                      # what step() does: gradients autograd kept outside the flat buffer are copied in
        total += opt.grad
    assert torch.allclose(g0, total, rtol=1e-5, atol=1e-6)


def test_bf16_gradient_exchange_gloo_world2():
    """AGAN_DP_BF16=1: buckets travel as bf16 and are summed in fp32 in rank order on arrival, the sum goes back as bf16
    (dataparallel.all_reduce_bf16_): both ranks end with  fp32(bf16(fp32(bf16(g0)) + fp32(bf16(g1))))  bit for bit -- within 2^-8 of
    the fp32 all-reduce."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, True)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(collect_from_children(q, procs, timeout=120), key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (_, s0, w0, g0, nb0), (_, s1, w1, g1, nb1) = got
    assert s0 == s1 == 0.5 and nb0 > 1 and torch.equal(w0, w1) and torch.equal(g0, g1)
    net = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 8), torch.nn.Linear(8, 8))
    opt = OPT.FlatAdam(net.parameters())
    with torch.no_grad():
        opt.flat.copy_(w0)
    shards = []
    for r in range(2):
        opt.zero_grad()
        net(torch.randn(4, 16, generator=torch.Generator().manual_seed(r))).pow(2).sum().backward()
        opt._rebind()
        shards.append(opt.grad.clone())
    want = (shards[0].to(torch.bfloat16).float() + shards[1].to(torch.bfloat16).float()).to(torch.bfloat16).float()
    assert torch.equal(g0, want)
    exact = shards[0] + shards[1]
    assert float((g0 - exact).abs().max()) <= 2.0 ** -7 * float(exact.abs().max())


def _tiny_step(seed=0):
    """GanTrainStep on CPU tensors: construction, checkpointing and the loop guard are host logic (the kernels never run here)"""
    torch.manual_seed(5)
    G = GEN.Generator(4, 16, 8, 8)
    Ds = [DISC.Disc64(4), DISC.Disc128(4), DISC.Disc256(4)]
    return TR.GanTrainStep(G, Ds, None, seed=seed)


def _ckpt_worker(rank, world, port, q, path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        step = _tiny_step(seed=3)
        draw = lambda st: torch.randn(6, generator=st.rng).numpy().copy()
        first = draw(step)                                  # some of the noise stream is consumed before the checkpoint
        sd = step.state_dict()                              # collective: every rank's generator state goes into ONE file
        assert set(sd["rng"]) == {0, 1} and set(sd["sample_rng"]) == {0, 1} and sd["rng_world"] == 2
        if rank == 0:
            torch.save(sd, path)
            solo = step.state_dict(all_ranks=False)         # rank-0-only pattern: no communication, its own state only
            torch.save(solo, path + ".solo")
            assert set(solo["rng"]) == {0}
        dist.barrier()
        after = draw(step)                                  # what the uninterrupted run draws next
        # resume: a fresh trainer (fresh seeds) on every rank loads the ONE file
        resumed = _tiny_step(seed=99)
        resumed.load_state_dict(torch.load(path, weights_only=True))
        got = draw(resumed)
        # rank-0-only checkpoint: rank 0 continues its stream, the other rank gets a derived -- different, deterministic -- one
        lone = _tiny_step(seed=99)
        lone.load_state_dict(torch.load(path + ".solo", weights_only=True))
        lone_draw = draw(lone)
        lone2 = _tiny_step(seed=7)
        lone2.load_state_dict(torch.load(path + ".solo", weights_only=True))
        q.put((rank, first, after, got, lone_draw, draw(lone2)))
    finally:
        dist.destroy_process_group()


def test_checkpoint_noise_streams_are_per_rank_gloo_world2(tmp_path):
    """one checkpoint file resumed by every rank must NOT give every rank rank 0's noise generator.
    state_dict() stores {rank: state}; load_state_dict() restores a rank's own state (bitwise resume on every rank) and derives a
    distinct deterministic one for a rank the file has no state for."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_ckpt_worker, args=(r, 2, port, q, str(tmp_path / "ckpt.pt"))) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(collect_from_children(q, procs, timeout=120), key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (_, f0, a0, g0, l0, l0b), (_, f1, a1, g1, l1, l1b) = got
    assert not np.array_equal(f0, f1) and not np.array_equal(a0, a1)          # replicas draw different noise (seed + rank)
    assert np.array_equal(g0, a0) and np.array_equal(g1, a1)                  # every rank resumes ITS stream bit for bit
    assert np.array_equal(l0, a0)                                             # rank-0-only file: rank 0 continues ...
    assert not np.array_equal(l1, a0) and not np.array_equal(l1, l0)          # ... rank 1 does not replay rank 0's noise
    assert np.array_equal(l1, l1b)                                            # and its derived stream does not depend on the new seed


def test_legacy_checkpoint_rng_entry_is_rank0s():
    """checkpoints written before the states were keyed by rank hold one bare generator state: rank 0 takes it as it is"""
    step = _tiny_step(seed=1)
    sd = step.state_dict()
    sd["rng"], sd["sample_rng"] = sd["rng"][0], sd["sample_rng"][0]
    want = torch.randn(4, generator=step.rng)
    other = _tiny_step(seed=2)
    other.load_state_dict(sd)
    assert torch.equal(torch.randn(4, generator=other.rng), want)
    g = torch.Generator()
    TR.GanTrainStep._restore_generator(g, sd["rng"], 3)                       # a higher rank: derived, not rank 0's
    assert not torch.equal(torch.randn(4, generator=g), want)


def _guard_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        step = _tiny_step()
        full = [5, 3, 2, 4]
        verdicts = [
            step.skip_batch(full, 4, 4),                                          # everyone fine -> run
            step.skip_batch([5, 1, 2, 4] if rank == 1 else full, 4, 4),           # a one-word caption on rank 1 only -> ALL skip
            step.skip_batch(full, 3 if rank == 0 else 4, 4),                      # a short last batch on rank 0 only -> ALL skip
            step.skip_batch(torch.tensor(full), 4, 4),                            # tensors of lengths are accepted
        ]
        q.put((rank, verdicts))
    finally:
        dist.destroy_process_group()


def test_batch_guard_is_decided_collectively_gloo_world2():
    """train.py:112 (`if min(lengths) < 2 or len(words) < BATCH_SIZE: continue`) under data parallelism: a rank skipping alone would
    deadlock the gradient all-reduce, so the verdict is one MAX all-reduce (dataparallel.any_rank) -- identical on every rank."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_guard_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(collect_from_children(q, procs, timeout=120), key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert got[0][1] == got[1][1] == [False, True, True, False]
    step = _tiny_step()                                                          # one rank: the reference's rule as written
    assert step.skip_batch([2, 2], 2, 2) is False and step.skip_batch([1, 2], 2, 2) is True and step.skip_batch([2], 1, 2) is True


def test_image_grid_helper(tmp_path):
    """trainers/trainer.py:68-98 as tensors: the largest square number of images, tiled row-major, per resolution"""
    t = TR.ModelTrainer()
    imgs = [torch.rand(11, 3, r, r) for r in (8, 16)]
    grids = t._image_grid(imgs)
    assert [tuple(g.shape) for g in grids] == [(3, 24, 24), (3, 48, 48)] and grids[0].dtype == torch.uint8      # 9 of 11 images, 3 x 3
    want = (imgs[0][5].clamp(0, 1) * 255.0 + 0.5).to(torch.uint8)                # image 5 sits in row 1, column 2
    assert torch.equal(grids[0][:, 8:16, 16:24], want)
    paths = t._plot_image_grid(imgs, epoch=2, folder=str(tmp_path))
    assert [os.path.basename(p) for p in paths] == ["epoch_2-8x8.ppm", "epoch_2-16x16.ppm"]
    head = open(paths[1], "rb").read(15)
    assert head.startswith(b"P6\n48 48\n255\n") and os.path.getsize(paths[1]) == len(b"P6\n48 48\n255\n") + 48 * 48 * 3


def test_stage1_generator_is_a_prefix_of_the_full_one():
    """Generator1 (BASELINE configs[1]) = the vae / gen1 / img_out1 submodules of Generator under the same names"""
    torch.manual_seed(3)
    full = GEN.Generator(4, 16, 8, 8)
    g1 = GEN.Generator1(4, 16, 8, 8)
    keys = {k for k in full.state_dict() if k.startswith(("vae.", "gen1.", "img_out1."))}
    assert set(g1.state_dict()) == keys
    g1.load_state_dict({k: v for k, v in full.state_dict().items() if k in keys})
    assert (g1.z_dim, g1.cond_dim) == (8, 8)


def test_bench_kernel_symbol_key():
    """bench.py / profiles/make_counters.py key per-kernel numbers with the rocprofv3 symbol minus return type, namespace and parameters"""
    sys.path.insert(0, ROOT)
    import bench
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import make_counters
    name = ("void (anonymous namespace)::conv_gather_f32_kernel<128, 128, 2, 2, 0>(float const*, float const*, float const*, void*, "
            "HIP_vector_type<int, 2u> const*, agan::conv::Geom, int, int, unsigned long, int, void const*)")
    for f in (bench.short_symbol, make_counters.short_symbol):
        assert f(name) == "conv_gather_f32_kernel<128, 128, 2, 2, 0>"
        assert f("(anonymous namespace)::conv_wino_h_f32_kernel(float const*, float const*, float*, agan::conv::Geom, agan::conv::WinoPlan)") == "conv_wino_h_f32_kernel"
    assert set(bench.WORKLOADS) == {"full3", "stage1_b64", "stage4_b8"}
    assert [bench.WORKLOADS[k]["config"] for k in ("stage1_b64", "full3", "stage4_b8")] == [1, 2, 4]


def test_bench_plain_run_leaves_side_measurements_to_full():
    """a plain `bench.py --gpus 1 --steps N --warmup W` times the headline only; roofline, variants and cpu_baseline need --full"""
    sys.path.insert(0, ROOT)
    import bench
    args = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not args.full and (args.workload, args.batch, args.precision) == ("full3", 24, "f32")
    assert bench.parse_args(["--full", "--layer-table", "t.txt"]).full
    with pytest.raises(SystemExit):
        bench.parse_args(["--layer-table", "t.txt"])


def test_golden_fixtures_are_data_only():
    for f in os.listdir(GOLDEN):
        if f.endswith(".npz"):
            z = np.load(os.path.join(GOLDEN, f), allow_pickle=False)
            assert all(z[k].dtype.kind in "fiub" for k in z.files), f


def test_encoder_plugins_on_cpu():
    """The frozen encoders are stock PyTorch modules (outside the hand-written scope): check the reference contract on CPU."""
    ENC = importlib.import_module("attention-gan_amd.networks.cnn_encoder")
    RNN = importlib.import_module("attention-gan_amd.networks.rnn_encoder")
    torch.manual_seed(0)
    r = RNN.RNNEncoder(vocabsize=30, nhidden=16)
    w, s = r(torch.randint(0, 30, (3, 5)), torch.tensor([5, 2, 4]))
    assert tuple(w.shape) == (3, 16, 5) and tuple(s.shape) == (3, 16)
    assert float(r.embedding.weight.abs().max()) <= 0.1
    assert {"embedding.weight", "rnn.weight_ih_l0", "rnn.weight_hh_l0_reverse"} <= set(r.state_dict())
    e = ENC.CNNEncoder(8)
    keys = set(e.state_dict())
    assert {"Conv2d_1a_3x3.conv.weight", "Mixed_5b.branch5x5_2.bn.running_var", "Mixed_6e.branch7x7dbl_5.conv.weight",
            "Mixed_7c.branch3x3dbl_3b.conv.weight", "emb_features.weight", "emb_cnn_code.bias"} <= keys
    assert sum(p.numel() for n, p in e.named_parameters() if not n.startswith("emb_")) == 21_785_568   # Inception-v3 trunk
    f, c = ENC.StandInImageEncoder(8)(torch.randn(2, 3, 64, 64))
    assert tuple(f.shape) == (2, 8, 17, 17) and tuple(c.shape) == (2, 8)


def _rnn_vs_golden(dev, tol):
    """f2: networks/rnn_encoder.py against the fixture generated from the reference's RNNEncoder (rnn_encoder.py:68-96)."""
    from helpers import assert_close, load, probe, sub, T
    RNN = importlib.import_module("attention-gan_amd.networks.rnn_encoder")
    g = load("f2_rnn_encoder")
    vocab, embdim, nhidden, B, Tn = (int(v) for v in g["dims"])
    m = RNN.RNNEncoder(vocabsize=vocab, embdim=embdim, dropprob=0.0, nhidden=nhidden)
    params = sub(g, "param/")
    assert set(m.state_dict()) == set(params)
    m.load_state_dict(params)
    m = m.to(dev).train()
    w, s = m(T(g["captions"]).to(dev), T(g["lengths"]))
    assert_close(w, g["word_embs"], tol, "word_embs")
    assert_close(s, g["sent_embs"], tol, "sent_embs")
    ((w * probe(w.shape, 0.7).to(dev)).sum() + (s * probe(s.shape, 0.8).to(dev)).sum()).backward()
    grads = sub(g, "gparam/")
    assert set(grads) == {k for k, p in m.named_parameters()}
    for k, p in m.named_parameters():
        assert_close(p.grad, grads[k], tol, f"grad {k}")


def test_rnn_encoder_vs_reference_golden_cpu():
    _rnn_vs_golden("cpu", 1e-5)


def test_batch_wire_format(tmp_path):
    BT = importlib.import_module("attention-gan_amd.data.batches")
    b = next(iter(BT.synthetic_batches(4, seq_len=6)))
    assert [tuple(t.shape) for t in b] == [(4, 6), (4,), (4,), (4, 3, 64, 64), (4, 3, 128, 128), (4, 3, 256, 256)]
    assert b[0].dtype == b[1].dtype == b[2].dtype == torch.int64 and b[3].dtype == torch.float32
    assert all(int((b[0][i, int(b[1][i]):] != 0).sum()) == 0 for i in range(4))
    rng = np.random.default_rng(0)
    n = 10
    lens = np.array([3, 5, 1, 4, 2, 6, 6, 2, 3, 4])
    BT.write_shard(str(tmp_path / "s.npz"), rng.integers(1, 9, (n, 6)), lens, rng.integers(0, 3, n),
                   *(rng.integers(0, 256, (n, 3, r, r), dtype=np.uint8) for r in (64, 128, 256)))
    got = list(BT.ShardBatches([str(tmp_path / "s.npz")], batch_size=4, shuffle=False))
    assert len(got) == 1                                   # first batch holds the 1-word caption -> skipped like train.py:112
    words, lengths, cids, i64, i128, i256 = got[0]
    assert lengths.tolist() == [2, 6, 6, 2] and words.shape == (4, 6)
    assert float(i256.min()) >= -1.0 and float(i256.max()) <= 1.0 and i64.shape == (4, 3, 64, 64)


def test_flat_buffer_epochs_are_per_buffer_and_survive_recycling():
    """packed-weight caches follow the Adam steps of THEIR flat buffer (functional.register_flat): ranges are looked up by
    address, an overlapping re-registration (recycled memory) drops the old range and starts above every epoch handed out, and a
    dropped range says that it is no longer registered."""
    HF = importlib.import_module("attention-gan_amd.backend.functional")
    saved = list(HF._FLAT_RANGES)
    try:
        HF._FLAT_RANGES[:] = []
        a, b = torch.zeros(100), torch.zeros(50)
        HF.register_flat(a)
        HF.register_flat(b)
        ra, rb = HF._flat_range(a.data_ptr() + 40), HF._flat_range(b.data_ptr())
        assert ra is not None and rb is not None and ra is not rb
        assert HF._flat_range(a.data_ptr() + 400) is not ra            # one past the end
        for _ in range(5):                                            # five optimiser steps on a
            HF.mark_flat_written(a)
        assert rb.epoch != ra.epoch
        assert ra.registered and rb.registered
        HF.register_flat(a[10:60])                                    # same memory handed out again under another base
        rn = HF._flat_range(a.data_ptr() + 44)
        assert rn is not ra and rn.epoch > ra.epoch and ra not in HF._FLAT_RANGES
        assert not ra.registered and rn.registered and rb.registered
        HF.unregister_flat(b)
        assert HF._flat_range(b.data_ptr()) is None and not rb.registered
    finally:
        HF._FLAT_RANGES[:] = saved


def test_rebind_keeps_autograd_sums_and_refuses_the_unrecoverable_case():
    """FlatAdam._rebind policy for a slice a backward KERNEL wrote while autograd ended up holding a tensor of its own
    (ADVICE r2): one kernel contribution -> autograd's tensor (a clone, or its sum with a stock edge of a tied weight) is the whole
    gradient and is copied in; several kernel contributions -> a clone equals the slice and is dropped, anything else raises."""
    HF = importlib.import_module("attention-gan_amd.backend.functional")
    lin = torch.nn.Linear(4, 3)
    opt = OPT.FlatAdam(lin.parameters())
    w = opt.params[0]
    dst = w._agan_grad_dst
    # -- one kernel edge + a stock edge summed by autograd (foreign tensor = kernel part + stock part)
    opt.zero_grad()
    buf, acc, handed = HF._grad_out(dst, w.shape, w)
    assert acc == 0 and handed.data_ptr() == opt.grad.data_ptr() + 4 * opt.offsets[0] and dst.edges == 1
    buf.fill_(1.0)                                              # "the kernel" writes the slice
    w.grad = handed + 2.0                                       # autograd's out-of-place sum with a stock edge
    assert opt._rebind([0]) == 1
    assert torch.equal(opt.grad[:w.numel()], torch.full((w.numel(),), 3.0)) and w.grad.data_ptr() == opt.grad.data_ptr()
    # -- two kernel edges, autograd cloned after both: equal to the slice -> dropped silently
    opt.zero_grad()
    buf, _, handed = HF._grad_out(dst, w.shape, w)
    buf.fill_(1.0)
    buf2, acc2, handed2 = HF._grad_out(dst, w.shape, w)
    assert acc2 == 1 and handed2 is None and dst.edges == 2
    buf2.add_(4.0)                                              # in-kernel accumulation of the second use
    w.grad = handed.clone()
    assert opt._rebind([0]) == 0 and torch.equal(opt.grad[:w.numel()], torch.full((w.numel(),), 5.0))
    # -- two kernel edges AND a stock edge summed with only the first: cannot be reconstructed -> refuse
    opt.zero_grad()
    buf, _, handed = HF._grad_out(dst, w.shape, w)
    buf.fill_(1.0)
    foreign = handed + 2.0
    HF._grad_out(dst, w.shape, w)[0].add_(4.0)
    w.grad = foreign
    with pytest.raises(RuntimeError, match="several in-kernel"):
        opt._rebind([0])


def test_bucket_lock_refuses_a_second_backward_into_an_exchanged_bucket():
    """Once a bucket has been handed to the gradient exchange no backward kernel may write into it until zero_grad()
    (without the old zero-fill a second backward would add into a bucket whose all-reduce is in flight)."""
    HF = importlib.import_module("attention-gan_amd.backend.functional")
    LIB = importlib.import_module("attention-gan_amd.backend.lib")
    lin = torch.nn.Linear(4, 3)
    opt = OPT.FlatAdam(lin.parameters())
    dst = opt.params[0]._agan_grad_dst
    opt.zero_grad()
    HF._grad_out(dst, opt.params[0].shape, opt.params[0])
    dst.locked = True                                           # what GradBuckets._launch does for the bucket's members
    with pytest.raises(LIB.AganError, match="already being all-reduced"):
        HF._grad_out(dst, opt.params[0].shape, opt.params[0])
    opt.zero_grad()
    assert not dst.locked and dst.edges == 0
    HF._grad_out(dst, opt.params[0].shape, opt.params[0])


def test_direct_rccl_chunk_arithmetic():
    """agan_allreduce_chunk_elems (pure host code of csrc/comm.hip): the reduce-scatter / all-gather split of a bucket -- equal,
    16-byte aligned chunks that tile the bucket exactly (rank r owns [r*chunk, (r+1)*chunk)), or 0 = library all-reduce."""
    lib = importlib.import_module("attention-gan_amd.backend.lib").load()
    for world in (1, 2, 4, 8):
        for n in (4, 8, 32, 1000, 1024, 4096 + 4, 16 << 20, (16 << 20) + 4, 7_084_592, 68_310_785, 12345):
            chunk = lib.agan_allreduce_chunk_elems(n, world)
            if n % world == 0 and (n // world) % 4 == 0:
                assert chunk == n // world and chunk * world == n and (chunk * 4) % 16 == 0
                offs = [r * chunk for r in range(world)]
                assert offs[-1] + chunk == n and all((o * 4) % 16 == 0 for o in offs)
            else:
                assert chunk == 0
    assert lib.agan_allreduce_chunk_elems(0, 8) == 0 and lib.agan_allreduce_chunk_elems(64, 0) == 0
    # the buckets GradBuckets cuts from a flat buffer are multiples of 4 elements (16-byte aligned parameters)
    mods = torch.nn.Sequential(*[torch.nn.Linear(33, 17) for _ in range(5)])
    opt = OPT.FlatAdam(mods.parameters())
    bk = DP.GradBuckets(opt, bucket_bytes=3000)
    assert all((e - s) % 4 == 0 and s % 4 == 0 for s, e in bk.bounds)
