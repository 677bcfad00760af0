"""CPU tests of the argument checks of the eight DAMSM entry points (include/agan.h: agan_func_attention_*, agan_words_loss_*,
agan_sent_loss_*): every one answers a shape outside its range, a missing required pointer or a short workspace with its error code
and a message naming it, before any device is touched -- forward and backward alike."""
import importlib

import pytest

L = importlib.import_module("attention-gan_amd.backend.lib")

P = 1                       # a non-null dummy pointer value: validation must fail before it is used
GOOD = (4, 64, 12, 289)     # B, D, T, S inside every range
# every dimension one step outside its range, the others good: B in [1,128], D and S in [1,320], T in [1,32]
BAD_WORDS = [(0, 64, 12, 289), (-3, 64, 12, 289), (129, 64, 12, 289), (4, 0, 12, 289), (4, -1, 12, 289), (4, 321, 12, 289),
             (4, 64, 0, 289), (4, 64, -2, 289), (4, 64, 33, 289), (4, 64, 12, 0), (4, 64, 12, -17), (4, 64, 12, 321)]
BIG = 1 << 40               # a workspace size that is never the reason for a refusal


def words_fwd(lib, dims, feat=P, wemb=P, lens=P, loss=P, sim=P, maps=P, save=P):
    return lib.agan_words_loss_fwd(feat, wemb, lens, None, None, 4.0, 5.0, 10.0, 5.0, loss, sim, maps, save, *dims, None)


def words_bwd(lib, dims, ws_bytes=BIG, feat=P, wemb=P, lens=P, save=P, dloss=P, dfeat=P, dwemb=P, ws=P):
    return lib.agan_words_loss_bwd(feat, wemb, lens, save, dloss, 4.0, 5.0, 10.0, 5.0, dfeat, dwemb, *dims, ws, ws_bytes, None)


def sent_fwd(lib, B, D, cnn=P, rnn=P, loss=P, save=P):
    return lib.agan_sent_loss_fwd(cnn, rnn, None, None, 10.0, 5.0, 1e-8, loss, save, B, D, None)


def sent_bwd(lib, B, D, cnn=P, rnn=P, save=P, dloss=P, dcnn=P, drnn=P):
    return lib.agan_sent_loss_bwd(cnn, rnn, save, dloss, 10.0, 5.0, 1e-8, dcnn, drnn, B, D, None)


def attn_fwd(lib, dims, query=P, context=P, wctx=P, attn=P):
    return lib.agan_func_attention_fwd(query, context, 4.0, 0.125, wctx, attn, *dims, None)


def attn_bwd(lib, dims, query=P, context=P, dwctx=P, dattn=P, dquery=P, dcontext=P):
    return lib.agan_func_attention_bwd(query, context, dwctx, dattn, 4.0, 0.125, dquery, dcontext, *dims, None)


@pytest.mark.parametrize("dims", BAD_WORDS, ids=lambda d: "B{}-D{}-T{}-S{}".format(*d))
def test_words_loss_entries_refuse_out_of_range_shapes(dims):
    lib = L.load()
    assert words_fwd(lib, dims) == L.EINVAL
    assert b"words_loss" in lib.agan_last_error()
    assert words_bwd(lib, dims) == L.EINVAL
    assert b"words_loss_bwd" in lib.agan_last_error()
    assert words_bwd(lib, dims, ws_bytes=0) == L.EINVAL         # not "workspace ok": the size query's 0 must not let the shape through
    assert b"words_loss_bwd" in lib.agan_last_error()
    assert words_fwd(lib, GOOD, feat=None) == L.EINVAL          # (leaves another message behind)
    assert lib.agan_words_loss_save_elems(*dims) == 0
    assert b"words_loss_save_elems" in lib.agan_last_error()
    if min(dims) <= 0:
        assert lib.agan_words_loss_bwd_ws_bytes(*dims) == 0


def test_words_loss_size_queries_inside_the_range():
    lib = L.load()
    B, D, T, S = GOOD
    assert lib.agan_words_loss_bwd_ws_bytes(B, D, T, S) == B * B * D * (S + T) * 4
    assert lib.agan_words_loss_save_elems(B, D, T, S) == B * B + B * D * S + B * D * 292      # MFMA form: + the padded features
    assert lib.agan_words_loss_save_elems(B, D, T, 290) == B * B + B * D * 290
    assert lib.agan_words_loss_save_elems(B, D, 13, S) == B * B + B * D * S
    assert lib.agan_words_loss_save_elems(B, 96, T, S) == B * B + B * 96 * S
    assert lib.agan_words_loss_save_elems(128, 320, 32, 320) == 128 * 128 + 128 * 320 * 320
    assert lib.agan_words_loss_bwd_ws_bytes(128, 320, 32, 320) == 128 * 128 * 320 * 352 * 4    # 7.4 GB: past 2^32 without wrapping


@pytest.mark.parametrize("missing", ["feat", "wemb", "lens", "loss", "sim", "maps", "save"])
def test_words_loss_fwd_refuses_null_pointers(missing):
    lib = L.load()
    assert words_fwd(lib, GOOD, **{missing: None}) == L.EINVAL
    assert b"words_loss_fwd: null pointer" in lib.agan_last_error()


@pytest.mark.parametrize("missing", ["feat", "wemb", "lens", "save", "dloss", "dfeat", "dwemb", "ws"])
def test_words_loss_bwd_refuses_null_pointers(missing):
    lib = L.load()
    assert words_bwd(lib, GOOD, **{missing: None}) == L.EINVAL
    assert b"words_loss_bwd: null pointer" in lib.agan_last_error()


def test_words_loss_bwd_refuses_a_short_workspace():
    lib = L.load()
    need = lib.agan_words_loss_bwd_ws_bytes(*GOOD)
    for short in (0, 4, need - 1):
        assert words_bwd(lib, GOOD, ws_bytes=short) == L.EWORKSPACE
        msg = lib.agan_last_error()
        assert b"words_loss_bwd: workspace" in msg and str(need).encode() in msg


@pytest.mark.parametrize("B,D", [(0, 64), (-1, 64), (129, 64), (4, 0), (4, -5)])
def test_sent_loss_entries_refuse_out_of_range_shapes(B, D):
    lib = L.load()
    assert sent_fwd(lib, B, D) == L.EINVAL
    assert b"sent_loss" in lib.agan_last_error()
    assert sent_bwd(lib, B, D) == L.EINVAL
    assert b"sent_loss_bwd" in lib.agan_last_error()


def test_sent_loss_entries_refuse_null_pointers():
    lib = L.load()
    for missing in ("cnn", "rnn", "loss", "save"):
        assert sent_fwd(lib, 4, 64, **{missing: None}) == L.EINVAL
        assert b"sent_loss_fwd: null pointer" in lib.agan_last_error()
    for missing in ("cnn", "rnn", "save", "dloss", "dcnn", "drnn"):
        assert sent_bwd(lib, 4, 64, **{missing: None}) == L.EINVAL
        assert b"sent_loss_bwd: null pointer" in lib.agan_last_error()


@pytest.mark.parametrize("dims", [(0, 32, 7, 25), (2, 0, 7, 25), (2, 321, 7, 25), (2, 32, 0, 25), (2, 32, 33, 25), (2, 32, 7, 0), (2, 32, 7, 321)],
                         ids=lambda d: "B{}-D{}-L{}-S{}".format(*d))
def test_func_attention_entries_refuse_out_of_range_shapes(dims):
    lib = L.load()
    assert attn_fwd(lib, dims) == L.EINVAL
    assert b"func_attention" in lib.agan_last_error()
    assert attn_bwd(lib, dims) == L.EINVAL
    assert b"func_attention_bwd" in lib.agan_last_error()


def test_func_attention_entries_refuse_null_pointers():
    lib = L.load()
    dims = (2, 32, 7, 25)
    for missing in ("query", "context", "wctx", "attn"):
        assert attn_fwd(lib, dims, **{missing: None}) == L.EINVAL
        assert b"func_attention_fwd: null pointer" in lib.agan_last_error()
    for missing in ("query", "context", "dquery", "dcontext"):          # dwctx / dattn are optional
        assert attn_bwd(lib, dims, **{missing: None}) == L.EINVAL
        assert b"func_attention_bwd: null pointer" in lib.agan_last_error()
