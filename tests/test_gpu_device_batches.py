"""agan_image_prep (csrc/batch_prep.hip) and the loader on top of it (data/batches.py: DeviceShardBatches) on the GPU.

Expected values: data.batches.scale_255_to_1 for direct planes (bit for bit), data.batches.downsample_reference for derived planes --
the integer restatement that tests/test_host_device_batches.py holds against torch's float64 antialiased bilinear resize to 1e-12 --
and ShardBatches for everything the loader yields.

Bound of the derived planes: |out - ref| <= 2^-23 absolute.  Outputs lie in [-1, 1], where a correctly rounded fp32 is within 2^-25
of the exact value, so the bound would leave two ulp of the top binade for an fp32 accumulation order.  The kernel does not use that
room: it forms the exact integer numerator and denominator and divides once, which is the correctly rounded fp32, and so is the
reference -- the tests also assert that the count of unequal elements is 0 (measured on an MI355X, plain and mirrored alike: 0 of 1 280 for 32x32, 0 of 1 200 for 24x40, 0 of
20 480 for the multi-band 128x256 case, 0 of 245 760 for the two batches of the 256-only shard; max |out - ref| = 0 everywhere)."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 2.0 ** -23

HF = importlib.import_module("attention-gan_amd.backend.functional")
BT = importlib.import_module("attention-gan_amd.data.batches")
GEN = importlib.import_module("attention-gan_amd.networks.generator")
DISC = importlib.import_module("attention-gan_amd.networks.discriminators")
ENC = importlib.import_module("attention-gan_amd.networks.cnn_encoder")
TR = importlib.import_module("attention-gan_amd.trainers.trainer")


def _u8(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _flags(v):
    return torch.tensor(v, dtype=torch.uint8, device=DEV)


def _expect_direct(src, rows, flip):
    """indexed, mirrored, scaled -- on the CPU with the reference's formula"""
    out = BT.scale_255_to_1(src[rows])
    for b, f in enumerate(flip):
        if f:
            out[b] = out[b].flip(-1)
    return out


def test_all_byte_values_scale_like_the_reference():
    src = torch.arange(256, dtype=torch.uint8).view(1, 1, 16, 16)
    (out,) = HF.image_prep([src.to(DEV)], None, None)
    assert out.dtype == torch.float32 and out.shape == (1, 1, 16, 16)
    assert torch.equal(out.cpu(), BT.scale_255_to_1(src))
    (narrow,) = HF.image_prep([src.view(1, 1, 32, 8).to(DEV)], None, None)               # rows shorter than a 16-byte chunk: pixel path
    assert torch.equal(narrow.cpu(), BT.scale_255_to_1(src.view(1, 1, 32, 8)))


def test_gather_and_flip_on_three_direct_planes():
    srcs = [_u8((5, 3, r, r), 10 + r) for r in (32, 16, 8)]
    dev = [s.to(DEV) for s in srcs]
    rows, flip = [4, 0, 2], [1, 0, 1]
    outs = HF.image_prep(dev, _i32(rows), _flags(flip))
    for s, o in zip(srcs, outs):
        assert torch.equal(o.cpu(), _expect_direct(s, rows, flip)), tuple(s.shape)
    again = HF.image_prep(dev, _i32(rows), _flags(flip))
    assert all(torch.equal(a, b) for a, b in zip(outs, again))                          # run to run
    # rows outside [0, n_src) give zeros and read nothing; sample 0 is intact
    given = [torch.full((3, 3, r, r), float("nan"), device=DEV) for r in (32, 16, 8)]
    outs = HF.image_prep(dev, _i32([0, 7, -1]), _flags(flip), out=given)
    for s, o, g in zip(srcs, outs, given):
        assert o.data_ptr() == g.data_ptr()
        assert torch.equal(o[0].cpu(), _expect_direct(s, [0], [1])[0])
        assert torch.equal(o[1:].cpu(), torch.zeros(2, 3, *s.shape[2:]))
    (no_flip,) = HF.image_prep(dev[:1], _i32(rows), None)
    assert torch.equal(no_flip.cpu(), _expect_direct(srcs[0], rows, [0, 0, 0]))


@pytest.mark.parametrize("mirror", [False, True], ids=["plain", "mirrored"])
@pytest.mark.parametrize("H,W,n_src,C", [(32, 32, 3, 2), (24, 40, 3, 2), (128, 256, 2, 1)], ids=["32x32", "24x40", "128x256-bands"])
def test_derived_planes_match_the_integer_restatement(H, W, n_src, C, mirror):
    """32x32 takes the 16-byte staging and store paths, 24x40 the byte staging and (6x10) the scalar stores; 128x256 cuts each derived
    plane into several bands (more than one block per image, halo rows shared between neighbours)."""
    src = _u8((n_src, C, H, W), H + W)
    rows = [n_src - 1, 0]
    flip = [1, 1] if mirror else None
    outs = HF.image_prep([src.to(DEV), (H // 2, W // 2), (H // 4, W // 4)], _i32(rows), _flags(flip) if mirror else None)
    picked = src[rows].flip(-1) if mirror else src[rows]
    assert torch.equal(outs[0].cpu(), BT.scale_255_to_1(picked))
    for o, f in zip(outs[1:], (2, 4)):
        ref = BT.downsample_reference(picked, f)
        assert o.shape == ref.shape
        err = float((o.cpu() - ref).abs().max())
        unequal = int((o.cpu() != ref).sum())
        print(f"{H}x{W} / {f} mirror={mirror}: max |out - ref| = {err:.3e}, unequal {unequal} of {ref.numel()}")
        assert err <= BOUND
        assert unequal == 0                     # one division of exact integers on both sides
    # mixed flags, and a sample outside the source: zeros in every plane
    outs = HF.image_prep([src.to(DEV), (H // 2, W // 2), (H // 4, W // 4)], _i32([1, n_src]), _flags([0, 1]))
    assert torch.equal(outs[1][0].cpu(), BT.downsample_reference(src[1], 2))
    assert all(float(o[1].abs().max()) == 0.0 for o in outs)
    again = HF.image_prep([src.to(DEV), (H // 2, W // 2), (H // 4, W // 4)], _i32([1, n_src]), _flags([0, 1]))
    assert all(torch.equal(a, b) for a, b in zip(outs, again))


def test_binding_refuses_host_tensors_and_wrong_types():
    L = importlib.import_module("attention-gan_amd.backend.lib")
    src = _u8((2, 1, 16, 16), 0)
    with pytest.raises(L.AganError, match="no CPU fallback"):
        HF.image_prep([src], None, None)
    with pytest.raises(L.AganError):
        HF.image_prep([src.to(DEV)], torch.zeros(2, dtype=torch.int64, device=DEV), None)
    with pytest.raises(L.AganError):
        HF.image_prep([src.to(DEV).float()], None, None)
    with pytest.raises(L.AganError, match="derived"):
        HF.image_prep([src.to(DEV), (5, 8)], None, None)


# ---- the loader --------------------------------------------------------------------------------------------------------------------
N, T, BS, SEED = 11, 6, 4, 3


def _write(path, seed, short_at, only256=False, n=N):
    """a shard with ONE caption of length 1, at sample `short_at`"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(2, T + 1, n)
    lens[short_at] = 1
    imgs = [rng.integers(0, 256, (n, 3, r, r), dtype=np.uint8) for r in (64, 128, 256)]
    words = rng.integers(1, 50, (n, T)) * (np.arange(T)[None, :] < lens[:, None])
    if only256:
        BT.write_shard(path, words, lens, rng.integers(0, 5, n), img256=imgs[2])
    else:
        BT.write_shard(path, words, lens, rng.integers(0, 5, n), *imgs)


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    """Two shards of N = 11, T = 6.  Under seed 3 the one-word caption of shard A sits in its first batch (skipped: A gives one batch)
    and that of shard B in the dropped tail of its permutation (B gives two)."""
    d = tmp_path_factory.mktemp("shards")
    rng = np.random.default_rng(SEED)
    perm_a, perm_b = rng.permutation(N), rng.permutation(N)
    a, b = str(d / "a.npz"), str(d / "b.npz")
    _write(a, 21, int(perm_a[0]))
    _write(b, 22, int(perm_b[N - 1]))
    solo_tail = int(np.random.default_rng(SEED).permutation(N)[N - 1])       # B alone: its permutation is the generator's first
    c = str(d / "c.npz")
    _write(c, 23, solo_tail)
    return dict(a=a, b=b, solo=c)


@pytest.fixture(scope="module")
def host_batches(shards):
    """ShardBatches' batches on the device, computed once and left unchanged"""
    both = list(BT.ShardBatches([shards["a"], shards["b"]], BS, device=DEV, shuffle=True, seed=SEED))
    solo = list(BT.ShardBatches([shards["solo"]], BS, device=DEV, shuffle=True, seed=SEED))
    assert len(both) == 3 and len(solo) == 2
    return dict(both=both, solo=solo)


def _checksum(batch):
    return torch.stack([t.double().sum() for t in batch] + [(batch[5].double() * torch.arange(256, device=DEV, dtype=torch.float64)).sum()])


def test_loader_yields_shard_batches_bit_for_bit(shards, host_batches):
    want = host_batches["both"]
    got = list(BT.DeviceShardBatches([shards["a"], shards["b"]], BS, DEV, shuffle=True, seed=SEED))
    assert len(got) == len(want)
    # (every batch kept without cloning: with three batches the first has seen the iterator advance twice and once more at its end;
    # the contract covers the last two, and the first still holds because its set is only rewritten by a fourth batch)
    for g, w in zip(got, want):
        assert len(g) == 6
        for a, b in zip(g, w):
            assert a.dtype == b.dtype and a.device == b.device and torch.equal(a, b)
    unshuffled = list(BT.DeviceShardBatches([shards["b"]], BS, DEV, shuffle=False))
    ref = list(BT.ShardBatches([shards["b"]], BS, device=DEV, shuffle=False))
    assert len(unshuffled) == len(ref) and all(torch.equal(a, b) for g, w in zip(unshuffled, ref) for a, b in zip(g, w))


def test_a_batch_stays_valid_after_one_advance(shards, host_batches):
    want = host_batches["both"]
    it = iter(BT.DeviceShardBatches([shards["a"], shards["b"]], BS, DEV, shuffle=True, seed=SEED))
    kept = next(it)                                   # not cloned
    nxt = next(it)
    for a, b in zip(kept, want[0]):
        assert torch.equal(a, b)
    for a, b in zip(nxt, want[1]):
        assert torch.equal(a, b)
    # each batch consumed by work enqueued AFTER the next next(): the sets are ordered by events, not by the host
    sums, prev = [], None
    for batch in BT.DeviceShardBatches([shards["a"], shards["b"]] * 3, BS, DEV, shuffle=True, seed=SEED):
        if prev is not None:
            sums.append(_checksum(prev))
        prev = batch
    sums.append(_checksum(prev))
    ref = [_checksum(b) for b in BT.ShardBatches([shards["a"], shards["b"]] * 3, BS, device=DEV, shuffle=True, seed=SEED)]
    assert len(sums) == len(ref) and len(ref) > BT.DeviceShardBatches.SETS          # every set has been rewritten at least once
    assert torch.equal(torch.stack(sums), torch.stack(ref))


def test_256_only_shard_derives_the_small_images(tmp_path):
    path = str(tmp_path / "only256.npz")
    _write(path, 31, short_at=4, only256=True, n=5)
    want = list(BT.ShardBatches([path], 2, device=DEV, shuffle=False))
    got = list(BT.DeviceShardBatches([path], 2, DEV, shuffle=False))
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert all(torch.equal(a, b) for a, b in zip(g[:3], w[:3])) and torch.equal(g[5], w[5])
        for k in (3, 4):
            assert g[k].shape == w[k].shape
            err, unequal = float((g[k] - w[k]).abs().max()), int((g[k] != w[k]).sum())
            print(f"256-only shard, image {k - 3}: max |out - ref| = {err:.3e}, unequal {unequal} of {w[k].numel()}")
            assert err <= BOUND and unequal == 0


def test_flip_prob_one_mirrors_every_image(shards, host_batches):
    got = list(BT.DeviceShardBatches([shards["solo"]], BS, DEV, shuffle=True, seed=SEED, flip_prob=1.0))
    want = host_batches["solo"]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert all(torch.equal(a, b) for a, b in zip(g[:3], w[:3]))
        assert all(torch.equal(a, b.flip(-1)) for a, b in zip(g[3:], w[3:]))
    # a fair coin mirrors some samples and not others, each either way exactly
    mixed = list(BT.DeviceShardBatches([shards["solo"]], BS, DEV, shuffle=True, seed=SEED, flip_prob=0.5))
    kinds = set()
    for g, w in zip(mixed, want):
        for s in range(BS):
            same, flipped = torch.equal(g[5][s], w[5][s]), torch.equal(g[5][s], w[5][s].flip(-1))
            assert same != flipped
            assert torch.equal(g[3][s], w[3][s].flip(-1) if flipped else w[3][s])
            kinds.add(flipped)
    assert kinds == {True, False}


def test_into_writes_the_static_buffers_of_a_graph(shards, host_batches):
    want = host_batches["solo"]
    static = [torch.zeros(BS, 3, r, r, device=DEV) for r in (64, 128, 256)]
    ptrs = [t.data_ptr() for t in static]
    it = iter(BT.DeviceShardBatches([shards["solo"]], BS, DEV, shuffle=True, seed=SEED, into=static))
    first = next(it)
    assert [t.data_ptr() for t in first[3:]] == ptrs
    total = lambda: torch.stack([t.double().sum() for t in static])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        total()                                        # warm-up off the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = total()
    for n, w in enumerate(want):
        batch = first if n == 0 else next(it)
        assert [t.data_ptr() for t in batch[3:]] == ptrs
        graph.replay()
        assert torch.allclose(out, torch.stack([t.double().sum() for t in w[3:]]), rtol=0, atol=1e-6), n
        assert all(torch.equal(a, b) for a, b in zip(batch, w)), n
    assert next(it, None) is None


def _train_two_steps(batches):
    torch.manual_seed(0)
    gf, df, emb, z, cond = 8, 8, 32, 16, 16
    G = GEN.Generator(gf, emb, z, cond).to(DEV)
    Ds = [DISC.Disc64(df).to(DEV), DISC.Disc128(df).to(DEV), DISC.Disc256(df).to(DEV)]
    enc = ENC.StandInImageEncoder(emb).to(DEV)
    enc.freeze_all_weights()
    table = torch.randn(50, emb, device=DEV)

    def text_encoder(words, lengths):
        e = table[words]                                                # [B, T, emb]
        return e.transpose(1, 2), e.mean(1)

    step = TR.GanTrainStep(G, Ds, enc, seed=0)
    assert step.train_epoch(batches, text_encoder, BS, max_batches=2) == 2
    torch.cuda.synchronize()
    return [torch.stack(h) for h in (step.d_losses, step.g_losses, step.damsm_losses)]


def test_train_epoch_is_bit_identical_under_both_loaders(shards):
    a = _train_two_steps(BT.ShardBatches([shards["solo"]], BS, device=DEV, shuffle=True, seed=SEED))
    b = _train_two_steps(BT.DeviceShardBatches([shards["solo"]], BS, DEV, shuffle=True, seed=SEED))
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.numel() == 2 and bool(torch.isfinite(x).all())
        assert torch.equal(x, y)
