"""The memory-contract table: one row per C-ABI function of include/ddrl.h that takes caller device memory (a *_d parameter, the host
arrays of device pointers src_h / out_h / region_base_h, the members of ddrl_rollout_nstep_out_t), naming the cases of
tests/test_gpu_abi_memory.py that hold it to the contract, and the closed list of exemptions with their reasons.
tests/test_abi_table_cpu.py parses the header against TABLE and EXEMPT: a new symbol fails there until it has a row or a stated reason.

A case is fn(ctx) -> call (tests/_abi_arena.py): it builds its handles from fixed seeds (so that the plain twin and every arena run
start from the same state), declares inputs with ctx.inp(name, array, ma=...) and outputs with ctx.out(name, elements, dtype, ma=...,
untouched=...) — extents as the header's comment states them, ma=True where the contract allows a pointer off the 16-byte grid — and
returns the closure that makes the call under test.  Where a call's effect stays inside a handle (store, import, set_state, adopt) the
closure reads it back through the export entry of the same family into an output, so that P2 / P4 see it."""
import ctypes
from ctypes import POINTER, byref, c_double, c_int32, c_int64, c_uint32, c_uint64, c_void_p as P

import numpy as np
import torch

F32, I32, I64, U8, F64 = torch.float32, torch.int32, torch.int64, torch.uint8, torch.float64

EXEMPT = {
    "ddrl_comm_bcast_params": "needs a communicator; world size 1 stays with tests/_rccl_world1_child.py",
    "ddrl_comm_allreduce_grads": "needs a communicator; world size 1 stays with tests/_rccl_world1_child.py",
    "ddrl_comm_send_batch": "needs a communicator; world size 1 stays with tests/_rccl_world1_child.py",
    "ddrl_comm_recv_batch": "needs a communicator; world size 1 stays with tests/_rccl_world1_child.py",
    "ddrl_replay_buffers": "returns addresses, writes no device memory",
    "ddrl_replay_buffers_ex": "returns addresses, writes no device memory",
    "ddrl_ps_buffer": "returns an address, writes no device memory",
    "ddrl_sac1_grad_buffer": "returns an address, writes no device memory",
    "ddrl_sac1_input_buffers": "returns addresses, writes no device memory",
    "ddrl_winq_buffers": "returns addresses, writes no device memory",
    "ddrl_dqn_step_timed": "profiling entry with host outputs; the kernels of ddrl_dqn_step, which has a row",
    "ddrl_sac1_stage_time": "profiling entry with a host output; the kernels of ddrl_sac1_step, which has a row",
}
# parameters of covered functions that are not caller DEVICE memory although the parse rule would not know
EXEMPT_PARAMS = {("ddrl_sac1_step_host", "block_h"): "page-locked host memory; losses_d of the same call is covered"}

CASES = {}   # id -> (fn, (functions covered))
TABLE = {}   # function -> [case ids]


def case(cid, *functions):
    def deco(fn):
        assert cid not in CASES, cid
        CASES[cid] = (fn, functions)
        for f in functions:
            TABLE.setdefault(f, []).append(cid)
        return fn
    return deco


# ---- small helpers ----------------------------------------------------------------------------------------------------------------
def _ok(ctx, rc):
    assert rc == 0, (rc, ctx.lib.ddrl_last_error())


def _dev(ctx):
    return ctx.device.index or 0


def _ptrs(*addrs):
    return (P * len(addrs))(*[P(a) for a in addrs])


def _tp(t):
    return P(t.data_ptr())


def _rs(seed):
    return np.random.RandomState(seed)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _handle(ctx, destroy, create, *args):
    h = P()
    _ok(ctx, create(byref(h), *args))
    ctx.defer(lambda: destroy(h))
    return h


# ---- rings ------------------------------------------------------------------------------------------------------------------------
CAP = 50
RING_SHAPES = {"o3a1": (3, 1, 0), "o8a2": (8, 2, 0), "o16a4u8": (16, 4, 2), "o20a1u8": (20, 1, 2)}   # obs, act, flags (2 = DDRL_REPLAY_U8_OBS)


def _rows5(obs, act, n, seed, u8):
    r = _rs(seed)
    ob = (lambda: _f32(r.randint(0, 256, (n, obs)))) if u8 else (lambda: _f32(r.randn(n, obs)))
    return [ob(), _f32(r.uniform(-1, 1, (n, act))), _f32(r.randn(n)), ob(), _f32(r.rand(n) < 0.2)]   # obs1, acts, rews, obs2, done


def _ring5(ctx, obs, act, flags=0, cap=CAP, fill=0, seed=3):
    L = ctx.lib
    h = _handle(ctx, L.ddrl_replay_destroy, L.ddrl_replay_create, _dev(ctx), cap, obs, act, flags)
    _ok(ctx, L.ddrl_replay_seed(h, seed, None))
    if fill:
        o1, a, r, o2, d = [ctx.tmp(x) for x in _rows5(obs, act, fill, 100 + seed, flags & 2)]
        _ok(ctx, L.ddrl_replay_store(h, _tp(o1), _tp(a), _tp(r), _tp(o2), _tp(d), fill, None))
    return h


def _export5(ctx, h, widths, cap, ma=False):
    """Closure part: the whole ring, array by array, into outputs ring0.. (ddrl_replay_rows_export)."""
    outs = [ctx.out("ring%d" % j, cap * w, F32, ma=ma) for j, w in enumerate(widths)]
    return lambda: [ctx.lib.ddrl_replay_rows_export(h, j, 0, cap, P(p), ctx.stream_arg) for j, p in enumerate(outs)]


def _mk_store(shape, n):
    obs, act, flags = RING_SHAPES[shape]

    def fn(ctx):
        h = _ring5(ctx, obs, act, flags, fill=7)       # cursor off 0, so that 64 rows wrap
        o1, a, r, o2, d = _rows5(obs, act, n, 5, flags & 2)
        p = [ctx.inp(k, x, ma=True) for k, x in (("obs_d", o1), ("act_d", a), ("rew_d", r), ("obs2_d", o2), ("done_d", d))]
        exp = _export5(ctx, h, (obs, obs, act, 1, 1), CAP)
        return lambda: [ctx.lib.ddrl_replay_store(h, P(p[0]), P(p[1]), P(p[2]), P(p[3]), P(p[4]), n, ctx.stream_arg)] + exp()
    return fn


for _s in RING_SHAPES:
    for _n in (1, 37, 64, 120):
        case("replay_store-%s-n%d" % (_s, _n), "ddrl_replay_store", "ddrl_replay_rows_export")(_mk_store(_s, _n))


def _mk_sample(shape, B, gather):
    obs, act, flags = RING_SHAPES[shape]

    def fn(ctx):
        L = ctx.lib
        h = _ring5(ctx, obs, act, flags, fill=37)
        o = [ctx.out(k, B * w, F32, ma=True) for k, w in (("obs1_d", obs), ("obs2_d", obs), ("acts_d", act), ("rews_d", 1), ("done_d", 1))]
        if gather:
            idx = ctx.inp("idx_d", _rs(B).randint(0, 37, B).astype(np.int64))
            return lambda: L.ddrl_replay_gather(h, P(idx), B, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), ctx.stream_arg)
        idx = ctx.out("idx_d", B, I64)
        return lambda: L.ddrl_replay_sample(h, B, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), P(idx), ctx.stream_arg)
    return fn


for _s in RING_SHAPES:
    for _b in (1, 37, 256):
        case("replay_sample-%s-B%d" % (_s, _b), "ddrl_replay_sample")(_mk_sample(_s, _b, False))
        case("replay_gather-%s-B%d" % (_s, _b), "ddrl_replay_gather")(_mk_sample(_s, _b, True))


@case("replay_sample-idx_null", "ddrl_replay_sample")
def _sample_idx_null(ctx):
    h = _ring5(ctx, 8, 2, fill=37)
    o = [ctx.out(k, 5 * w, F32) for k, w in (("obs1_d", 8), ("obs2_d", 8), ("acts_d", 2), ("rews_d", 1), ("done_d", 1))]
    return lambda: ctx.lib.ddrl_replay_sample(h, 5, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), None, ctx.stream_arg)


@case("replay_sample-empty_ring_refused", "ddrl_replay_sample")
def _sample_refused(ctx):
    """DDRL_ERR_EMPTY_BUFFER: a refused call leaves its outputs alone."""
    h = _ring5(ctx, 8, 2)
    ctx.expect_rc = -2
    o = [ctx.out(k, 5 * w, F32, untouched=True) for k, w in (("obs1_d", 8), ("obs2_d", 8), ("acts_d", 2), ("rews_d", 1), ("done_d", 1))]
    idx = ctx.out("idx_d", 5, I64, untouched=True)
    return lambda: ctx.lib.ddrl_replay_sample(h, 5, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), P(idx), ctx.stream_arg)


@case("replay_sample_indices", "ddrl_replay_sample_indices")
def _sample_indices(ctx):
    h = _ring5(ctx, 8, 2, fill=37)
    idx = ctx.out("idx_d", 37, I64)
    return lambda: ctx.lib.ddrl_replay_sample_indices(h, 37, P(idx), ctx.stream_arg)


@case("replay_take_error", "ddrl_replay_take_error")
def _take_error(ctx):
    h = _ring5(ctx, 8, 2, fill=5)
    w = ctx.out("out_d", 1, I32)
    return lambda: ctx.lib.ddrl_replay_take_error(h, P(w), ctx.stream_arg)


def _mk_rows(shape, imp):
    obs, act, flags = RING_SHAPES[shape]

    def fn(ctx):
        L = ctx.lib
        h = _ring5(ctx, obs, act, flags, fill=37)
        if imp:
            src = ctx.inp("src_d", _rows5(obs, act, 7, 9, flags & 2)[0], ma=True)
            exp = _export5(ctx, h, (obs, obs, act, 1, 1), CAP)
            return lambda: [L.ddrl_replay_rows_import(h, 0, 3, 7, P(src), ctx.stream_arg)] + exp()
        out = ctx.out("out_d", 7 * obs, F32, ma=True)
        return lambda: L.ddrl_replay_rows_export(h, 1, 3, 7, P(out), ctx.stream_arg)
    return fn


for _s in RING_SHAPES:
    case("replay_rows_export-%s" % _s, "ddrl_replay_rows_export")(_mk_rows(_s, False))
    case("replay_rows_import-%s" % _s, "ddrl_replay_rows_import")(_mk_rows(_s, True))


def _mk_sample_many(shape):
    obs, act, flags = RING_SHAPES[shape]

    def fn(ctx):
        h = _ring5(ctx, obs, act, flags, fill=37)
        o = [ctx.out("out_h[%d]" % j, 3 * 5 * w, F32, ma=True) for j, w in enumerate((obs, obs, act, 1, 1))]
        arr = _ptrs(*o)
        return lambda: ctx.lib.ddrl_replay_sample_many(h, 5, 3, arr, ctx.stream_arg)
    return fn


for _s in RING_SHAPES:
    case("replay_sample_many-%s" % _s, "ddrl_replay_sample_many")(_mk_sample_many(_s))


# ---- window rings (Ln, obs): the generalised entries and the n-step fold --------------------------------------------------------------
WINDOWS = {"Ln1o8": (1, 8), "Ln3o5": (3, 5), "Ln8o8": (8, 8)}
WACT, GAMMA = 2, 0.99


def _wwidths(Ln, obs):
    return ((Ln + 1) * obs, Ln * WACT, Ln, Ln)


def _wrows(Ln, obs, n, seed):
    r = _rs(seed)
    w = _wwidths(Ln, obs)
    return [_f32(r.randn(n, w[0])), _f32(r.uniform(-1, 1, (n, w[1]))), _f32(r.randn(n, w[2])), _f32(r.rand(n, w[3]) < 0.2)]


def _wring(ctx, Ln, obs, fill=0, seed=3, cap=CAP):
    L = ctx.lib
    w = (ctypes.c_int32 * 4)(*_wwidths(Ln, obs))
    h = _handle(ctx, L.ddrl_replay_destroy, L.ddrl_replay_create_ex, _dev(ctx), cap, 4, w, 1, 1)
    _ok(ctx, L.ddrl_replay_seed(h, seed, None))
    if fill:
        t = [ctx.tmp(x) for x in _wrows(Ln, obs, fill, 100 + seed)]
        _ok(ctx, L.ddrl_replay_store_ex(h, _ptrs(*[x.data_ptr() for x in t]), fill, None))
    return h


def _mk_store_ex(win, n, mask):
    Ln, obs = WINDOWS[win]

    def fn(ctx):
        L = ctx.lib
        h = _wring(ctx, Ln, obs, fill=7)
        src = _ptrs(*[ctx.inp("src_h[%d]" % j, x, ma=True) for j, x in enumerate(_wrows(Ln, obs, n, 5))])
        exp = _export5(ctx, h, _wwidths(Ln, obs), CAP)
        if mask is None:
            return lambda: [L.ddrl_replay_store_ex(h, src, n, ctx.stream_arg)] + exp()
        m = np.zeros(n, np.uint8)
        if mask == "one":
            m[n // 2] = 1
        elif mask == "all":
            m[:] = 1
        md = ctx.inp("mask_d", m)
        return lambda: [L.ddrl_replay_store_masked_ex(h, src, P(md), n, ctx.stream_arg)] + exp()
    return fn


for _w in WINDOWS:
    for _n in (1, 37, 64, 120):
        case("replay_store_ex-%s-n%d" % (_w, _n), "ddrl_replay_store_ex")(_mk_store_ex(_w, _n, None))
    for _m in ("none", "one", "all"):
        case("replay_store_masked_ex-%s-%s" % (_w, _m), "ddrl_replay_store_masked_ex")(_mk_store_ex(_w, 37, _m))


def _mk_sample_ex(win, B, mode):
    Ln, obs = WINDOWS[win]

    def fn(ctx):
        L = ctx.lib
        h = _wring(ctx, Ln, obs, fill=37)
        if mode in ("sample_ex", "gather_ex"):
            o = _ptrs(*[ctx.out("out_h[%d]" % j, B * w, F32, ma=True) for j, w in enumerate(_wwidths(Ln, obs))])
            if mode == "gather_ex":
                idx = ctx.inp("idx_d", _rs(B).randint(0, 37, B).astype(np.int64))
                return lambda: L.ddrl_replay_gather_ex(h, P(idx), B, o, ctx.stream_arg)
            idx = ctx.out("idx_d", B, I64)
            return lambda: L.ddrl_replay_sample_ex(h, B, o, P(idx), ctx.stream_arg)
        names = (("obs1_d", obs), ("obs2_d", obs), ("acts_d", WACT), ("rews_d", 1), ("done_d", 1))
        if mode == "sample_nstep":
            o = [ctx.out(k, B * w, F32, ma=True) for k, w in names]
            idx = ctx.out("idx_d", B, I64)
            return lambda: L.ddrl_replay_sample_nstep(h, B, GAMMA, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), P(idx), ctx.stream_arg)
        o = _ptrs(*[ctx.out("out_h[%d]" % j, 3 * B * w, F32, ma=True) for j, (_, w) in enumerate(names)])
        return lambda: L.ddrl_replay_sample_many_nstep(h, B, 3, GAMMA, o, ctx.stream_arg)
    return fn


for _w in WINDOWS:
    for _b in (1, 37, 256):
        case("replay_sample_ex-%s-B%d" % (_w, _b), "ddrl_replay_sample_ex")(_mk_sample_ex(_w, _b, "sample_ex"))
        case("replay_sample_nstep-%s-B%d" % (_w, _b), "ddrl_replay_sample_nstep")(_mk_sample_ex(_w, _b, "sample_nstep"))
    case("replay_gather_ex-%s" % _w, "ddrl_replay_gather_ex")(_mk_sample_ex(_w, 37, "gather_ex"))
    case("replay_sample_many_nstep-%s" % _w, "ddrl_replay_sample_many_nstep")(_mk_sample_ex(_w, 5, "sample_many_nstep"))


def _mk_fold(win, B):
    Ln, obs = WINDOWS[win]

    def fn(ctx):
        w = [ctx.inp(k, x, ma=True) for k, x in zip(("obs_w_d", "acts_w_d", "rews_w_d", "done_w_d"), _wrows(Ln, obs, B, 11))]
        o = [ctx.out(k, B * n, F32, ma=True) for k, n in (("obs1_d", obs), ("obs2_d", obs), ("acts_d", WACT), ("rews_d", 1), ("done_d", 1))]
        return lambda: ctx.lib.ddrl_nstep_fold(P(w[0]), P(w[1]), P(w[2]), P(w[3]), B, Ln, obs, WACT, GAMMA,
                                               P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), ctx.stream_arg)
    return fn


for _w in WINDOWS:
    for _b in (1, 37):
        case("nstep_fold-%s-B%d" % (_w, _b), "ddrl_nstep_fold")(_mk_fold(_w, _b))


@case("replay_set_feed", "ddrl_replay_set_feed", "ddrl_replay_sample_ex")
def _set_feed(ctx):
    """Plan [batch 1 of region 0, local draw]: the fed entry copies a block batch and leaves idx_d untouched, the local one draws."""
    L, B, W = ctx.lib, 5, (8, 8, 2, 1, 1)
    owner = _ring5(ctx, 8, 2, fill=37, seed=5)
    blk = ctx.tmp(np.zeros(3 * B * sum(W), np.float32))
    offs = np.cumsum([0] + [3 * B * w for w in W])
    _ok(ctx, L.ddrl_replay_sample_many(owner, B, 3, _ptrs(*[blk.data_ptr() + 4 * int(o) for o in offs[:5]]), None))
    ctx.sync()
    h = _ring5(ctx, 8, 2, fill=37)
    plan = ctx.inp("plan_d", np.array([0 << 24 | 1, -1], np.int32))
    base = _ptrs(ctx.inp("region_base_h[0]", blk.cpu().numpy(), ma=True))
    cnt = (ctypes.c_int32 * 1)(3)
    fed = _ptrs(*[ctx.out("fed.out_h[%d]" % j, B * w, F32) for j, w in enumerate(W)])
    fed_idx = ctx.out("fed.idx_d", B, I64, untouched=True)
    loc = _ptrs(*[ctx.out("local.out_h[%d]" % j, B * w, F32) for j, w in enumerate(W)])
    loc_idx = ctx.out("local.idx_d", B, I64)

    def call():
        rcs = [L.ddrl_replay_set_feed(h, P(plan), 2, B, 1, base, cnt, ctx.stream_arg), L.ddrl_replay_sample_ex(h, B, fed, P(fed_idx), ctx.stream_arg),
               L.ddrl_replay_sample_ex(h, B, loc, P(loc_idx), ctx.stream_arg)]
        ctx.sync()
        return rcs + [L.ddrl_replay_set_feed(h, None, 0, B, 0, None, None, ctx.stream_arg)]
    return call


# ---- parameter server -----------------------------------------------------------------------------------------------------------------
PS_N = 100


def _mk_ps(off, cnt, pull):
    def fn(ctx):
        L = ctx.lib
        h = _handle(ctx, L.ddrl_ps_destroy, L.ddrl_ps_create, _dev(ctx), PS_N)
        base = ctx.tmp(_f32(_rs(1).randn(PS_N)))
        _ok(ctx, L.ddrl_ps_push(h, _tp(base), 0, PS_N, None))
        if pull:
            dst = ctx.out("dst_d", cnt, F32, ma=True)
            return lambda: L.ddrl_ps_pull(h, P(dst), off, cnt, ctx.stream_arg)
        src = ctx.inp("src_d", _f32(_rs(2).randn(cnt)), ma=True)
        allp = ctx.out("server", PS_N, F32)
        return lambda: [L.ddrl_ps_push(h, P(src), off, cnt, ctx.stream_arg), L.ddrl_ps_pull(h, P(allp), 0, PS_N, ctx.stream_arg)]
    return fn


for _o, _c in ((0, PS_N), (1, 5), (PS_N - 3, 3)):
    case("ps_push-off%d-n%d" % (_o, _c), "ddrl_ps_push", "ddrl_ps_pull")(_mk_ps(_o, _c, False))
    case("ps_pull-off%d-n%d" % (_o, _c), "ddrl_ps_pull")(_mk_ps(_o, _c, True))


# ---- counter noise --------------------------------------------------------------------------------------------------------------------
def _mk_fill(n, uniform):
    ctr = (1 << 32) - 100      # the counter's low word wraps inside the n = 255 / 257 fills

    def fn(ctx):
        o = ctx.out("out_d", n, F32, ma=True)
        if uniform:
            return lambda: ctx.lib.ddrl_uniform_fill(P(o), n, -1.0, 1.0, 7, ctr, ctx.stream_arg)
        return lambda: ctx.lib.ddrl_normal_fill(P(o), n, 7, ctr, ctx.stream_arg)
    return fn


for _n in (1, 255, 257):
    case("normal_fill-n%d" % _n, "ddrl_normal_fill")(_mk_fill(_n, False))
    case("uniform_fill-n%d" % _n, "ddrl_uniform_fill")(_mk_fill(_n, True))


# ---- SAC1 / SAC-v learner ---------------------------------------------------------------------------------------------------------------
SAC_SHAPES = {"o8a2h64x48B37": (8, 2, 64, 48, 37), "o3a1h36x8B5": (3, 1, 36, 8, 5)}


def _sac_counts(o, a, h1, h2, variant):
    pi = o * h1 + h1 + h1 * h2 + h2 + 2 * (h2 * a + a)
    q = (o + a) * h1 + h1 + h1 * h2 + h2 + h2 + 1
    v = o * h1 + h1 + h1 * h2 + h2 + h2 + 1
    return pi, pi + 2 * q + (v if variant else 0)


def _sac_cfg(shape, variant=0, batch=None):
    from distributed_drl_amd import _lib
    o, a, h1, h2, B = SAC_SHAPES[shape]
    return _lib.Sac1Config(obs_dim=o, act_dim=a, hidden1=h1, hidden2=h2, batch=batch or B, variant=variant, lr=1e-3)


def _weights(n, seed):
    return _f32(_rs(seed).randn(n) * 0.2)


def _sac(ctx, shape, variant=0, seed=21):
    L = ctx.lib
    cfg = _sac_cfg(shape, variant)
    h = _handle(ctx, L.ddrl_sac1_destroy, L.ddrl_sac1_create, _dev(ctx), byref(cfg))
    o, a, h1, h2, B = SAC_SHAPES[shape]
    n = _sac_counts(o, a, h1, h2, variant)[1]
    _ok(ctx, L.ddrl_sac1_set_weights(h, _tp(ctx.tmp(_weights(n, seed))), None))
    return h, n


def _sac_batch(shape, seed):
    o, a, _, _, B = SAC_SHAPES[shape]
    r = _rs(seed)
    return [("obs1_d", _f32(r.randn(B, o))), ("obs2_d", _f32(r.randn(B, o))), ("acts_d", _f32(r.uniform(-1, 1, (B, a)))),
            ("rews_d", _f32(r.randn(B))), ("done_d", _f32(r.rand(B) < 0.2)), ("eps_x_d", _f32(r.randn(B, a))),
            ("eps_x2_d", _f32(r.randn(B, a))), ("eps_t_d", _f32(r.randn(B, a)))]


def _mk_sac_step(shape, variant, grads, rows):
    B = SAC_SHAPES[shape][4]

    def fn(ctx):
        L = ctx.lib
        h, n = _sac(ctx, shape, variant)
        ins = [P(ctx.inp(k, x)) for k, x in _sac_batch(shape, 31)]
        losses = P(ctx.out("losses_d", 4 if variant else 3, F32))
        per = [P(ctx.out(k, B, F32)) if rows else None for k in ("q1_d", "q2_d", "logp_pi_d")]
        exp = [(w, P(ctx.out("export%d" % w, n, F32))) for w in ((4,) if grads else (0, 1, 2, 3))]
        f = L.ddrl_sac1_compute_grads if grads else L.ddrl_sac1_step
        return lambda: [f(h, *ins, losses, *per, ctx.stream_arg)] + [L.ddrl_sac1_export(h, w, p, ctx.stream_arg) for w, p in exp]
    return fn


for _s in SAC_SHAPES:
    for _v, _vn in ((0, "sac1"), (1, "sacv")):
        case("%s_step-%s-rows" % (_vn, _s), "ddrl_sac1_step", "ddrl_sac1_export")(_mk_sac_step(_s, _v, False, True))
        case("%s_step-%s-rows_null" % (_vn, _s), "ddrl_sac1_step", "ddrl_sac1_export")(_mk_sac_step(_s, _v, False, False))
        case("%s_compute_grads-%s" % (_vn, _s), "ddrl_sac1_compute_grads", "ddrl_sac1_export")(_mk_sac_step(_s, _v, True, True))


def _mk_sac_io(shape, variant, mode):
    def fn(ctx):
        L = ctx.lib
        h, n = _sac(ctx, shape, variant)
        if mode == "get_weights":
            o = ctx.out("flat_main_d", n, F32, ma=True)
            return lambda: L.ddrl_sac1_get_weights(h, P(o), ctx.stream_arg)
        if mode == "set_weights":
            src = ctx.inp("flat_main_d", _weights(n, 77), ma=True)
            o = [P(ctx.out("export%d" % w, n, F32)) for w in (0, 1)]
            return lambda: [L.ddrl_sac1_set_weights(h, P(src), ctx.stream_arg)] + [L.ddrl_sac1_export(h, w, p, ctx.stream_arg) for w, p in enumerate(o)]
        which = int(mode[-1])
        if mode.startswith("export"):
            ins = [_tp(ctx.tmp(x)) for _, x in _sac_batch(shape, 31)]      # one update first: moments, target and gradient are not the initial ones
            _ok(ctx, L.ddrl_sac1_step(h, *ins, _tp(ctx.tmp(np.zeros(4, np.float32))), None, None, None, None))
            o = ctx.out("flat_d", n, F32, ma=True)
            return lambda: L.ddrl_sac1_export(h, which, P(o), ctx.stream_arg)
        src = ctx.inp("flat_d", np.abs(_weights(n, 78)) if which == 3 else _weights(n, 78), ma=True)
        o = ctx.out("export", n, F32)
        return lambda: [L.ddrl_sac1_import(h, which, P(src), ctx.stream_arg), L.ddrl_sac1_export(h, which, P(o), ctx.stream_arg)]
    return fn


for _s in SAC_SHAPES:
    for _m in ("get_weights", "set_weights") + tuple("export%d" % w for w in range(5)) + tuple("import%d" % w for w in range(4)):
        _f = {"g": "ddrl_sac1_get_weights", "s": "ddrl_sac1_set_weights", "e": "ddrl_sac1_export", "i": "ddrl_sac1_import"}[_m[0]]
        case("sac1_%s-%s" % (_m, _s), _f)(_mk_sac_io(_s, 0, _m))
case("sacv_set_weights", "ddrl_sac1_set_weights")(_mk_sac_io("o8a2h64x48B37", 1, "set_weights"))
case("sacv_get_weights", "ddrl_sac1_get_weights")(_mk_sac_io("o8a2h64x48B37", 1, "get_weights"))


def _mk_sac_step_host(shape):
    o, a, h1, h2, B = SAC_SHAPES[shape]

    def fn(ctx):
        L = ctx.lib
        h, n = _sac(ctx, shape)
        bufs = (P * 8)()
        _ok(ctx, L.ddrl_sac1_input_buffers(h, 0, bufs))
        p = [int(bufs[i]) for i in range(5)]
        off = [(x - p[0]) // 4 for x in p]
        span = off[4] + B
        host = ctx.keep(torch.zeros(span + 2, dtype=torch.float32).pin_memory())
        hv = host.numpy()
        for j, (_, x) in enumerate(_sac_batch(shape, 31)[:5]):
            hv[off[j]:off[j] + x.size] = x.reshape(-1)
        losses = ctx.out("losses_d", 3, F32)
        exp = [P(ctx.out("export%d" % w, n, F32)) for w in (0, 2)]
        return lambda: [L.ddrl_sac1_step_host(h, P(host.data_ptr()), span, 5, 1000, P(losses), ctx.stream_arg)] + [
            L.ddrl_sac1_export(h, w, e, ctx.stream_arg) for w, e in zip((0, 2), exp)]
    return fn


for _s in SAC_SHAPES:
    case("sac1_step_host-%s" % _s, "ddrl_sac1_step_host")(_mk_sac_step_host(_s))


# ---- actors ---------------------------------------------------------------------------------------------------------------------------
ACTOR_SHAPE, MAX_ROWS = "o8a2h64x48B37", 64


def _actor(ctx, shape=ACTOR_SHAPE, max_rows=MAX_ROWS, seed=41):
    L = ctx.lib
    cfg = _sac_cfg(shape)
    h = _handle(ctx, L.ddrl_actor_destroy, L.ddrl_actor_create, _dev(ctx), byref(cfg), max_rows)
    o, a, h1, h2, _ = SAC_SHAPES[shape]
    n_pi = _sac_counts(o, a, h1, h2, 0)[0]
    _ok(ctx, L.ddrl_actor_set_weights(h, _tp(ctx.tmp(_weights(n_pi, seed))), None))
    return h, n_pi


def _mk_actor_act(shape, n, det):
    o, a = SAC_SHAPES[shape][:2]

    def fn(ctx):
        h, _ = _actor(ctx, shape)
        r = _rs(n)
        obs = ctx.inp("obs_d", _f32(r.randn(n, o)), ma=True)
        eps = None if det else ctx.inp("eps_d", _f32(r.randn(n, a)), ma=True)
        act = ctx.out("act_d", n * a, F32, ma=True)       # the rows of act_d beyond n are guard, not extent
        return lambda: ctx.lib.ddrl_actor_act(h, P(obs), P(eps) if eps else None, n, det, P(act), ctx.stream_arg)
    return fn


for _s in SAC_SHAPES:
    for _n in (1, 5, 33):
        case("actor_act-%s-n%d" % (_s, _n), "ddrl_actor_act")(_mk_actor_act(_s, _n, 0))
    case("actor_act-%s-deterministic" % _s, "ddrl_actor_act")(_mk_actor_act(_s, 5, 1))


def _mk_actor_one(shape, det):
    o, a = SAC_SHAPES[shape][:2]

    def fn(ctx):
        h, _ = _actor(ctx, shape)
        obs = ctx.inp("obs_d", _f32(_rs(4).randn(o)), ma=True)
        act = ctx.out("act_d", a, F32, ma=True)
        return lambda: ctx.lib.ddrl_actor_act_one(h, P(obs), 9, (1 << 32) - 1, det, P(act), ctx.stream_arg)
    return fn


for _s in SAC_SHAPES:
    case("actor_act_one-%s" % _s, "ddrl_actor_act_one")(_mk_actor_one(_s, 0))
case("actor_act_one-deterministic", "ddrl_actor_act_one")(_mk_actor_one(ACTOR_SHAPE, 1))


def _mk_actor_weights(setw):
    def fn(ctx):
        L = ctx.lib
        h, n_pi = _actor(ctx)
        if setw:
            src = ctx.inp("flat_pi_d", _weights(n_pi, 79), ma=True)
            o = ctx.out("get_weights", n_pi, F32)
            return lambda: [L.ddrl_actor_set_weights(h, P(src), ctx.stream_arg), L.ddrl_actor_get_weights(h, P(o), ctx.stream_arg)]
        o = ctx.out("flat_pi_d", n_pi, F32, ma=True)
        return lambda: L.ddrl_actor_get_weights(h, P(o), ctx.stream_arg)
    return fn


case("actor_set_weights", "ddrl_actor_set_weights", "ddrl_actor_get_weights")(_mk_actor_weights(True))
case("actor_get_weights", "ddrl_actor_get_weights")(_mk_actor_weights(False))


def _versioned_actor(ctx):
    """Two versions live: envs 0, 3, 40 have adopted the second install, the others act on the first."""
    L = ctx.lib
    h, n_pi = _actor(ctx)
    _ok(ctx, L.ddrl_actor_versions_enable(h, 8, None))
    _ok(ctx, L.ddrl_actor_set_weights(h, _tp(ctx.tmp(_weights(n_pi, 43))), None))
    ended = np.zeros(MAX_ROWS, np.uint8)
    ended[[0, 3, 40]] = 1
    return h, ended


@case("actor_act_versioned", "ddrl_actor_act_versioned")
def _act_versioned(ctx):
    L = ctx.lib
    h, ended = _versioned_actor(ctx)
    _ok(ctx, L.ddrl_actor_versions_adopt(h, _tp(ctx.tmp(ended)), MAX_ROWS, None))
    r = _rs(6)
    obs, eps = ctx.inp("obs_d", _f32(r.randn(MAX_ROWS, 8)), ma=True), ctx.inp("eps_d", _f32(r.randn(MAX_ROWS, 2)), ma=True)
    act = ctx.out("act_d", MAX_ROWS * 2, F32, ma=True)
    return lambda: L.ddrl_actor_act_versioned(h, P(obs), P(eps), MAX_ROWS, 0, 1000, P(act), ctx.stream_arg)


@case("actor_versions_adopt_and_state", "ddrl_actor_versions_adopt", "ddrl_actor_versions_state")
def _versions_adopt(ctx):
    L = ctx.lib
    h, ended = _versioned_actor(ctx)
    e = ctx.inp("ended_d", ended)
    slots = ctx.out("slot_of_env_d", MAX_ROWS, I32)
    st = ctx.keep((ctypes.c_int32 * 4)())
    return lambda: [L.ddrl_actor_versions_adopt(h, P(e), MAX_ROWS, ctx.stream_arg), L.ddrl_actor_versions_state(h, P(slots), st, ctx.stream_arg)]


# ---- evaluation -----------------------------------------------------------------------------------------------------------------------
EPISODES, EP_LEN = 3, 6


def _mk_policy_eval(trace):
    def fn(ctx):
        cfg = ctx.keep(_sac_cfg(ACTOR_SHAPE))
        n_pi = _sac_counts(8, 2, 64, 48, 0)[0]
        w = ctx.inp("pi_flat_d", _weights(n_pi, 41))
        ret, ln = ctx.out("ret_d", EPISODES, F64), ctx.out("len_d", EPISODES, I32)
        tr = ctx.out("trace_d", EPISODES * EP_LEN * 12, F32) if trace else None     # rows past an episode's end: zeros (header)
        return lambda: ctx.lib.ddrl_policy_eval(byref(cfg), P(w), EPISODES, 5, 2, EP_LEN, P(ret), P(ln), P(tr) if tr else None, ctx.stream_arg)
    return fn


case("policy_eval-trace", "ddrl_policy_eval")(_mk_policy_eval(True))
case("policy_eval-trace_null", "ddrl_policy_eval")(_mk_policy_eval(False))


# ---- envs -----------------------------------------------------------------------------------------------------------------------------
ENV_N = (1, 33, 257)
MODELS = {"one_body": None, "articulated": (1, 4, 2)}


def _env(ctx, n, model, seed=7, max_ep_len=2):
    """max_ep_len 2 and one step taken: the step under test hits the time limit, so every env also goes through its reset."""
    from distributed_drl_amd import _lib
    L = ctx.lib
    m = MODELS[model]
    em = _lib.EnvModel(*m) if m else None
    h = _handle(ctx, L.ddrl_env_destroy, L.ddrl_env_create_ex, _dev(ctx), n, seed, max_ep_len, byref(em) if em else None)
    return h, L.ddrl_env_state_fields(h)


def _env_warm(ctx, h, n, discrete=False):
    L = ctx.lib
    if discrete:
        _ok(ctx, L.ddrl_env_step_discrete(h, _tp(ctx.tmp(_f32(_rs(1).randint(0, 4, n)))), None, None, None, None, None, None))
    else:
        _ok(ctx, L.ddrl_env_step(h, _tp(ctx.tmp(_f32(_rs(1).uniform(-1, 1, (n, 2))))), None, None, None, None, None, None))


def _env_outs(ctx, n, present):
    if not present:
        return [None] * 5
    return [P(ctx.out("obs2_d", n * 8, F32)), P(ctx.out("rew_d", n, F32)), P(ctx.out("done_d", n, F32)),
            P(ctx.out("next_obs_d", n * 8, F32)), P(ctx.out("ended_d", n, U8))]


def _mk_env_step(model, n, kind, present):
    def fn(ctx):
        L = ctx.lib
        h, fields = _env(ctx, n, model)
        _env_warm(ctx, h, n, kind == "discrete")
        if kind == "discrete":
            act = ctx.inp("act_idx_d", _f32(_rs(2).randint(0, 4, n)))
        else:
            act = ctx.inp("act_d", _f32(_rs(2).uniform(-1.2, 1.2, (n, 2))), modified=kind == "wrapped")
        outs = _env_outs(ctx, n, present)
        st = P(ctx.out("state_d", fields * n, F32))
        if kind == "wrapped":
            return lambda: [L.ddrl_env_step_wrapped(h, P(act), 0.3, 0.1, 5.0, 2, 2, *outs, ctx.stream_arg), L.ddrl_env_get_state(h, st, ctx.stream_arg)]
        f = L.ddrl_env_step_discrete if kind == "discrete" else L.ddrl_env_step
        return lambda: [f(h, P(act), *outs, ctx.stream_arg), L.ddrl_env_get_state(h, st, ctx.stream_arg)]
    return fn


for _m in MODELS:
    for _n in ENV_N:
        for _p in (True, False):
            _t = "" if _p else "-outputs_null"
            case("env_step-%s-n%d%s" % (_m, _n, _t), "ddrl_env_step", "ddrl_env_get_state")(_mk_env_step(_m, _n, "step", _p))
            case("env_step_discrete-%s-n%d%s" % (_m, _n, _t), "ddrl_env_step_discrete")(_mk_env_step(_m, _n, "discrete", _p))
            if _m == "one_body":
                case("env_step_wrapped-n%d%s" % (_n, _t), "ddrl_env_step_wrapped")(_mk_env_step(_m, _n, "wrapped", _p))


def _mk_env_reset(model, n, mask, obs):
    def fn(ctx):
        L = ctx.lib
        h, fields = _env(ctx, n, model, max_ep_len=100)
        _env_warm(ctx, h, n)
        m = P(ctx.inp("mask_d", (np.arange(n) % 3 == 0).astype(np.uint8))) if mask else None
        o = P(ctx.out("obs_d", n * 8, F32)) if obs else None
        st = P(ctx.out("state_d", fields * n, F32))
        return lambda: [L.ddrl_env_reset(h, m, o, ctx.stream_arg), L.ddrl_env_get_state(h, st, ctx.stream_arg)]
    return fn


for _m in MODELS:
    for _n in ENV_N:
        case("env_reset-%s-n%d" % (_m, _n), "ddrl_env_reset")(_mk_env_reset(_m, _n, False, True))
        case("env_reset-%s-n%d-mask" % (_m, _n), "ddrl_env_reset")(_mk_env_reset(_m, _n, True, True))
    case("env_reset-%s-obs_null" % _m, "ddrl_env_reset")(_mk_env_reset(_m, 33, True, False))


def _mk_env_state(model, n):
    def fn(ctx):
        L = ctx.lib
        h, fields = _env(ctx, n, model)
        h2, _ = _env(ctx, n, model, seed=8)
        _env_warm(ctx, h2, n)
        src = ctx.tmp(torch.empty(fields * n, dtype=torch.float32))
        _ok(ctx, L.ddrl_env_get_state(h2, _tp(src), None))
        ctx.sync()
        s = P(ctx.inp("state_d(set)", src.cpu().numpy(), ma=True))
        o = P(ctx.out("state_d(get)", fields * n, F32, ma=True))
        return lambda: [L.ddrl_env_set_state(h, s, ctx.stream_arg), L.ddrl_env_get_state(h, o, ctx.stream_arg)]
    return fn


for _m in MODELS:
    for _n in ENV_N:
        case("env_set_get_state-%s-n%d" % (_m, _n), "ddrl_env_set_state", "ddrl_env_get_state")(_mk_env_state(_m, _n))


# ---- fused rollout steps ----------------------------------------------------------------------------------------------------------------
RN, RCAP = 64, 200


def _mk_rollout(model, n_steps, act_m, obs_m):
    def fn(ctx):
        L = ctx.lib
        h, fields = _env(ctx, RN, model, max_ep_len=3)
        a, _ = _actor(ctx)
        ring = _ring5(ctx, 8, 2, cap=RCAP, fill=7)
        begin, step = ((L.ddrl_rollout_begin_articulated, L.ddrl_rollout_step_articulated) if model == "articulated"
                       else (L.ddrl_rollout_begin, L.ddrl_rollout_step))
        _ok(ctx, begin(h, a, None))
        _ok(ctx, step(h, a, ring, 2, 5, 0, 0, None, None, None))      # two steps taken: the steps under test meet the time limit
        am = P(ctx.out("act_out_d", RN * 2, F32)) if act_m else None
        om = P(ctx.out("next_obs_out_d", RN * 8, F32)) if obs_m else None
        st = P(ctx.out("state_d", fields * RN, F32))
        exp = _export5(ctx, ring, (8, 8, 2, 1, 1), RCAP)
        return lambda: [step(h, a, ring, n_steps, 5, 1000, 0, am, om, ctx.stream_arg), L.ddrl_env_get_state(h, st, ctx.stream_arg)] + exp()
    return fn


for _m, _f in (("one_body", "ddrl_rollout_step"), ("articulated", "ddrl_rollout_step_articulated")):
    for _k in (1, 2):
        for _a, _o in ((1, 1), (1, 0), (0, 1), (0, 0)):
            case("rollout_step-%s-steps%d-act%d-obs%d" % (_m, _k, _a, _o), _f)(_mk_rollout(_m, _k, _a, _o))


def _mk_rollout_nstep(n_steps, present):
    Ln = 4

    def fn(ctx):
        from distributed_drl_amd import _lib
        L = ctx.lib
        h, fields = _env(ctx, RN, "one_body", max_ep_len=1 << 20)
        a, _ = _actor(ctx)
        ring = _wring(ctx, Ln, 8, cap=RCAP)
        q = _handle(ctx, L.ddrl_winq_destroy, L.ddrl_winq_create, _dev(ctx), RN, Ln, 8, 2, 1)
        obs = ctx.tmp(torch.empty(RN * 8, dtype=torch.float32))
        _ok(ctx, L.ddrl_env_reset(h, None, _tp(obs), None))
        _ok(ctx, L.ddrl_winq_begin(q, None, _tp(obs), None))
        _ok(ctx, L.ddrl_rollout_begin_nstep(h, a, q, None))
        args = (0.3, 0.1, 5.0, 2, 3, 0, 5)
        _ok(ctx, L.ddrl_rollout_step_nstep(h, a, q, ring, 4, *args, 0, None, None))     # four steps: the windows are full, episodes end
        names = (("act", 2, F32), ("obs2", 8, F32), ("rew", 1, F32), ("done", 1, F32), ("next_obs", 8, F32), ("ended", 1, U8))
        out = ctx.keep(_lib.RolloutNStepOut(*[P(ctx.out("out->" + k, RN * w, t)) if k in present else None for k, w, t in names]))
        st = P(ctx.out("state_d", fields * RN, F32))
        exp = _export5(ctx, ring, _wwidths(Ln, 8), RCAP)
        return lambda: [L.ddrl_rollout_step_nstep(h, a, q, ring, n_steps, *args, 4000, byref(out) if present else None, ctx.stream_arg),
                        L.ddrl_env_get_state(h, st, ctx.stream_arg)] + exp()
    return fn


_ALL6 = ("act", "obs2", "rew", "done", "next_obs", "ended")
for _k in (1, 2):
    case("rollout_step_nstep-steps%d-all_mirrors" % _k, "ddrl_rollout_step_nstep")(_mk_rollout_nstep(_k, _ALL6))
    case("rollout_step_nstep-steps%d-out_null" % _k, "ddrl_rollout_step_nstep")(_mk_rollout_nstep(_k, ()))
for _one in _ALL6:
    case("rollout_step_nstep-only_%s" % _one, "ddrl_rollout_step_nstep")(_mk_rollout_nstep(1, (_one,)))
    case("rollout_step_nstep-without_%s" % _one, "ddrl_rollout_step_nstep")(_mk_rollout_nstep(1, tuple(k for k in _ALL6 if k != _one)))


def _mk_winq(win, push):
    Ln, obs = WINDOWS[win]
    n = 37

    def fn(ctx):
        from distributed_drl_amd.replay import _view
        L = ctx.lib
        q = _handle(ctx, L.ddrl_winq_destroy, L.ddrl_winq_create, _dev(ctx), n, Ln, obs, WACT, 1)
        arrs, tq = (P * 4)(), P()
        _ok(ctx, L.ddrl_winq_buffers(q, arrs, byref(tq)))
        r = _rs(3)
        if push:
            _ok(ctx, L.ddrl_winq_begin(q, None, _tp(ctx.tmp(_f32(r.randn(n, obs)))), None))
            for _ in range(Ln - 1):
                t = [ctx.tmp(_f32(r.randn(n, w))) for w in (obs, WACT, 1, 1)]
                _ok(ctx, L.ddrl_winq_push(q, *[_tp(x) for x in t], _tp(ctx.tmp(np.zeros(n, np.uint8))), None))
            ins = [P(ctx.inp(k, _f32(r.randn(n, w)))) for k, w in (("obs2_d", obs), ("act_d", WACT), ("rew_d", 1), ("done_d", 1))]
            ready = P(ctx.out("ready_d", n, U8))
            call = lambda: L.ddrl_winq_push(q, *ins, ready, ctx.stream_arg)
        else:
            m = P(ctx.inp("mask_d", (np.arange(n) % 2).astype(np.uint8)))
            o = P(ctx.inp("obs_d", _f32(r.randn(n, obs))))
            call = lambda: L.ddrl_winq_begin(q, m, o, ctx.stream_arg)
        # the queues live in the handle: the closure copies the observation windows and t_queue (int32 bits) out, device to device
        ctx.out("o_queue", n * (Ln + 1) * obs, F32)
        ctx.out("t_queue", n, F32)

        def run():
            rc = call()
            ctx.tensor("o_queue").copy_(_view(arrs[0], (n * (Ln + 1) * obs,), ctx.device))
            ctx.tensor("t_queue").copy_(_view(tq.value, (n,), ctx.device))
            return rc
        return run
    return fn


for _w in WINDOWS:
    case("winq_begin-%s" % _w, "ddrl_winq_begin")(_mk_winq(_w, False))
    case("winq_push-%s" % _w, "ddrl_winq_push")(_mk_winq(_w, True))


# ---- Double-DQN / SQN -------------------------------------------------------------------------------------------------------------------
DQN_SHAPES = {"o8A2h64x48B37": (8, 2, 64, 48, 37), "o3A1h36x8B5": (3, 1, 36, 8, 5), "o1028A2h64x48B37": (1028, 2, 64, 48, 37),
              "o8A4h64x48B64": (8, 4, 64, 48, 64)}
VARIANTS = {"ddqn": 0, "sqn": 1}


def _dqn_cfg(shape, variant):
    from distributed_drl_amd import _lib
    o, A, h1, h2, B = DQN_SHAPES[shape]
    return _lib.DqnConfig(o, A, h1, h2, B, variant=variant)


def _dqn(ctx, shape, variant=0, seed=51):
    L = ctx.lib
    cfg = ctx.keep(_dqn_cfg(shape, variant))
    n = ctypes.c_int64()
    _ok(ctx, L.ddrl_dqn_param_count(byref(cfg), byref(n)))
    h = _handle(ctx, L.ddrl_dqn_destroy, L.ddrl_dqn_create, _dev(ctx), byref(cfg))
    _ok(ctx, L.ddrl_dqn_set_weights(h, _tp(ctx.tmp(_weights(n.value, seed) * 0.25)), None))
    return h, int(n.value), cfg


def _dqn_batch(shape, seed):
    o, A, _, _, B = DQN_SHAPES[shape]
    r = _rs(seed)
    return [("obs1_d", _f32(r.randn(B, o))), ("obs2_d", _f32(r.randn(B, o))), ("acts_d", _f32(r.randint(0, A, B))),
            ("rews_d", _f32(r.randn(B))), ("done_d", _f32(r.rand(B) < 0.2))]


def _mk_dqn_step(shape, variant, outs):
    o, A, _, _, B = DQN_SHAPES[shape]

    def fn(ctx):
        L = ctx.lib
        h, n, _ = _dqn(ctx, shape, variant)
        # wide observations: 16-byte aligned rows are read in place, rows off that grid are staged (the header's words) — both run
        ins = [P(ctx.inp(k, x, ma=(o >= 1024 and k in ("obs1_d", "obs2_d")))) for k, x in _dqn_batch(shape, 61)]
        loss = P(ctx.out("loss_d", 1, F32)) if outs else None
        q = P(ctx.out("q_d", B * A, F32)) if outs else None
        exp = [(w, P(ctx.out("export%d" % w, n, F32))) for w in (0, 1, 2, 3, 4)]
        return lambda: [L.ddrl_dqn_step(h, *ins, loss, q, ctx.stream_arg)] + [L.ddrl_dqn_export(h, w, p, ctx.stream_arg) for w, p in exp]
    return fn


for _s in ("o8A2h64x48B37", "o3A1h36x8B5", "o1028A2h64x48B37"):
    for _vn, _v in VARIANTS.items():
        if _s.startswith("o1028") and _v:
            continue
        case("%s_step-%s" % (_vn, _s), "ddrl_dqn_step", "ddrl_dqn_export")(_mk_dqn_step(_s, _v, True))
        case("%s_step-%s-outputs_null" % (_vn, _s), "ddrl_dqn_step", "ddrl_dqn_export")(_mk_dqn_step(_s, _v, False))


def _mk_dqn_io(shape, variant, mode):
    def fn(ctx):
        L = ctx.lib
        h, n, _ = _dqn(ctx, shape, variant)
        if mode == "set_weights":
            src = ctx.inp("flat_main_d", _weights(n, 80) * 0.25, ma=True)
            o = [P(ctx.out("export%d" % w, n, F32)) for w in (0, 1)]
            return lambda: [L.ddrl_dqn_set_weights(h, P(src), ctx.stream_arg)] + [L.ddrl_dqn_export(h, w, p, ctx.stream_arg) for w, p in enumerate(o)]
        which = int(mode[-1])
        if mode.startswith("export"):
            ins = [_tp(ctx.tmp(x)) for _, x in _dqn_batch(shape, 61)]      # one update first: moments, target and gradient are not the initial ones
            _ok(ctx, L.ddrl_dqn_step(h, *ins, None, None, None))
            o = ctx.out("flat_d", n, F32, ma=True)
            return lambda: L.ddrl_dqn_export(h, which, P(o), ctx.stream_arg)
        src = ctx.inp("flat_d", np.abs(_weights(n, 81)) if which == 3 else _weights(n, 81), ma=True)
        o = ctx.out("export", n, F32)
        return lambda: [L.ddrl_dqn_import(h, which, P(src), ctx.stream_arg), L.ddrl_dqn_export(h, which, P(o), ctx.stream_arg)]
    return fn


for _s in ("o8A2h64x48B37", "o3A1h36x8B5"):
    for _vn, _v in VARIANTS.items():
        for _m in ("set_weights",) + tuple("export%d" % w for w in range(5)) + tuple("import%d" % w for w in range(4)):
            _f = {"s": "ddrl_dqn_set_weights", "e": "ddrl_dqn_export", "i": "ddrl_dqn_import"}[_m[0]]
            case("%s_%s-%s" % (_vn, _m, _s), _f)(_mk_dqn_io(_s, _v, _m))


def _mk_dqn_q(shape, variant, n, act):
    o, A, _, _, B = DQN_SHAPES[shape]

    def fn(ctx):
        L = ctx.lib
        h, _, _ = _dqn(ctx, shape, variant)
        obs = P(ctx.inp("obs_d", _f32(_rs(n).randn(n, o)), ma=True))
        if act is None:
            q = P(ctx.out("q_d", n * A, F32, ma=True))
            return lambda: L.ddrl_dqn_q(h, obs, n, q, ctx.stream_arg)
        a = P(ctx.out("act_d", n, F32, ma=True))
        q = P(ctx.out("q_out_d", n * A, F32, ma=True)) if act == "q" else None
        return lambda: L.ddrl_dqn_act(h, obs, n, 0, 0.5, 9, (1 << 32) - 2, a, q, ctx.stream_arg)
    return fn


for _s in ("o8A2h64x48B37", "o3A1h36x8B5"):
    for _vn, _v in VARIANTS.items():
        for _n in sorted({1, 2, DQN_SHAPES[_s][4] - 1}):
            case("%s_q-%s-n%d" % (_vn, _s, _n), "ddrl_dqn_q")(_mk_dqn_q(_s, _v, _n, None))
            case("%s_act-%s-n%d" % (_vn, _s, _n), "ddrl_dqn_act")(_mk_dqn_q(_s, _v, _n, "q"))
        case("%s_act-%s-q_null" % (_vn, _s), "ddrl_dqn_act")(_mk_dqn_q(_s, _v, 2, "noq"))


def _mk_dqn_step_ring(outs):
    shape = "o1028A2h64x48B37"
    o, A, _, _, B = DQN_SHAPES[shape]

    def fn(ctx):
        L = ctx.lib
        h, n, _ = _dqn(ctx, shape, 0)
        ring = _ring5(ctx, o, 1, 0, fill=0)
        r = _rs(71)
        rows = [_f32(r.randn(CAP, o)), _f32(r.randint(0, A, (CAP, 1))), _f32(r.randn(CAP)), _f32(r.randn(CAP, o)), _f32(r.rand(CAP) < 0.2)]
        _ok(ctx, L.ddrl_replay_store(ring, *[_tp(ctx.tmp(x)) for x in rows], CAP, None))
        loss = P(ctx.out("loss_d", 1, F32)) if outs else None
        q = P(ctx.out("q_d", B * A, F32)) if outs else None
        idx = P(ctx.out("idx_out_d", B, I64)) if outs else None
        exp = [(w, P(ctx.out("export%d" % w, n, F32))) for w in (0, 2)]
        return lambda: [L.ddrl_dqn_step_ring(h, ring, loss, q, idx, ctx.stream_arg)] + [L.ddrl_dqn_export(h, w, p, ctx.stream_arg) for w, p in exp]
    return fn


case("ddqn_step_ring", "ddrl_dqn_step_ring")(_mk_dqn_step_ring(True))
case("ddqn_step_ring-outputs_null", "ddrl_dqn_step_ring")(_mk_dqn_step_ring(False))


def _mk_dqn_loop(variant, loss):
    shape = "o8A2h64x48B37"
    o, A, _, _, B = DQN_SHAPES[shape]

    def fn(ctx):
        L = ctx.lib
        h, n, _ = _dqn(ctx, shape, variant)
        ring = _ring5(ctx, o, 1, 0, fill=0)
        r = _rs(72)
        rows = [_f32(r.randn(CAP, o)), _f32(r.randint(0, A, (CAP, 1))), _f32(r.randn(CAP)), _f32(r.randn(CAP, o)), _f32(r.rand(CAP) < 0.2)]
        _ok(ctx, L.ddrl_replay_store(ring, *[_tp(ctx.tmp(x)) for x in rows], CAP, None))
        ld = P(ctx.out("loss_d", 1, F32)) if loss else None
        loop = _handle(ctx, L.ddrl_dqn_loop_destroy, L.ddrl_dqn_loop_create, h, ring, 2, ld)   # updates_per_graph 2: loss_d is baked into the graphs
        exp = [(w, P(ctx.out("export%d" % w, n, F32))) for w in (0, 2)]
        return lambda: [L.ddrl_dqn_loop_run(loop, 5, ctx.stream_arg)] + [L.ddrl_dqn_export(h, w, p, ctx.stream_arg) for w, p in exp]
    return fn


for _vn, _v in VARIANTS.items():
    case("%s_loop-loss" % _vn, "ddrl_dqn_loop_create")(_mk_dqn_loop(_v, True))
case("ddqn_loop-loss_null", "ddrl_dqn_loop_create")(_mk_dqn_loop(0, False))


DSHAPE = "o8A4h64x48B64"


@case("dqn_versions_adopt_and_state", "ddrl_dqn_versions_adopt", "ddrl_dqn_versions_state")
def _dqn_versions(ctx):
    L = ctx.lib
    h, n, _ = _dqn(ctx, DSHAPE)
    _ok(ctx, L.ddrl_dqn_versions_enable(h, 8, None))
    _ok(ctx, L.ddrl_dqn_set_weights(h, _tp(ctx.tmp(_weights(n, 53) * 0.25)), None))
    ended = np.zeros(64, np.uint8)
    ended[[0, 3, 40]] = 1
    e = ctx.inp("ended_d", ended)
    slots = ctx.out("slot_of_env_d", 64, I32)
    st = ctx.keep((ctypes.c_int32 * 4)())
    return lambda: [L.ddrl_dqn_versions_adopt(h, P(e), 64, ctx.stream_arg), L.ddrl_dqn_versions_state(h, P(slots), st, ctx.stream_arg)]


def _mk_rollout_discrete(variant, n_steps, present):
    def fn(ctx):
        L = ctx.lib
        h, fields = _env(ctx, RN, "one_body", max_ep_len=3)
        d, _, _ = _dqn(ctx, DSHAPE, variant)
        ring = _ring5(ctx, 8, 1, cap=RCAP, fill=7)
        _ok(ctx, L.ddrl_rollout_begin_discrete(h, d, None))
        _ok(ctx, L.ddrl_rollout_step_discrete(h, d, ring, 2, 0, 0.5, 5, 0, None, None, None, None))
        am = P(ctx.out("act_out_d", RN, F32)) if "act" in present else None
        qm = P(ctx.out("q_out_d", RN * 4, F32)) if "q" in present else None
        om = P(ctx.out("next_obs_out_d", RN * 8, F32)) if "obs" in present else None
        st = P(ctx.out("state_d", fields * RN, F32))
        exp = _export5(ctx, ring, (8, 8, 1, 1, 1), RCAP)
        return lambda: [L.ddrl_rollout_step_discrete(h, d, ring, n_steps, 0, 0.5, 5, 1000, am, qm, om, ctx.stream_arg),
                        L.ddrl_env_get_state(h, st, ctx.stream_arg)] + exp()
    return fn


for _vn, _v in VARIANTS.items():
    for _k in (1, 2):
        case("rollout_step_discrete-%s-steps%d-all_mirrors" % (_vn, _k), "ddrl_rollout_step_discrete")(_mk_rollout_discrete(_v, _k, ("act", "q", "obs")))
for _p in ((), ("act",), ("q",), ("obs",)):
    case("rollout_step_discrete-mirrors_%s" % ("+".join(_p) or "null"), "ddrl_rollout_step_discrete")(_mk_rollout_discrete(0, 1, _p))


def _mk_dqn_eval(variant, mode, trace):
    shape = "o8A4h64x48B64"

    def fn(ctx):
        cfg = ctx.keep(_dqn_cfg(shape, variant))
        n = ctypes.c_int64()
        _ok(ctx, ctx.lib.ddrl_dqn_param_count(byref(cfg), byref(n)))
        w = ctx.inp("q_flat_d", _weights(n.value, 51) * 0.25)
        ret, ln = ctx.out("ret_d", EPISODES, F64), ctx.out("len_d", EPISODES, I32)
        tr = ctx.out("trace_d", EPISODES * EP_LEN * 20, F32) if trace else None
        return lambda: ctx.lib.ddrl_dqn_eval(byref(cfg), P(w), EPISODES, 5, 2, EP_LEN, mode, 0.5, 9, 100, P(ret), P(ln),
                                             P(tr) if tr else None, ctx.stream_arg)
    return fn


for _vn, _v in VARIANTS.items():
    case("%s_eval-trace" % _vn, "ddrl_dqn_eval")(_mk_dqn_eval(_v, 0, True))
    case("%s_eval-trace_null" % _vn, "ddrl_dqn_eval")(_mk_dqn_eval(_v, 1, False))


# ---- section 4: the env family's vector-moved pointers are refused one float off their grid, on the host -----------------------------
# (function, pointer named by ddrl_last_error()); tests/test_gpu_abi_memory.py makes each call with exactly that pointer offset by 4 bytes
REFUSALS = [
    ("ddrl_env_reset", "obs_d"),
    ("ddrl_env_step", "act_d"), ("ddrl_env_step", "obs2_d"), ("ddrl_env_step", "next_obs_d"),
    ("ddrl_env_step_discrete", "obs2_d"), ("ddrl_env_step_discrete", "next_obs_d"),
    ("ddrl_env_step_wrapped", "act_d"), ("ddrl_env_step_wrapped", "obs2_d"), ("ddrl_env_step_wrapped", "next_obs_d"),
    ("ddrl_rollout_step", "act_out_d"), ("ddrl_rollout_step", "next_obs_out_d"),
    ("ddrl_rollout_step_articulated", "act_out_d"), ("ddrl_rollout_step_articulated", "next_obs_out_d"),
    ("ddrl_rollout_step_discrete", "next_obs_out_d"),
    ("ddrl_rollout_step_nstep", "out->act"), ("ddrl_rollout_step_nstep", "out->obs2"), ("ddrl_rollout_step_nstep", "out->next_obs"),
    ("ddrl_policy_eval", "trace_d"), ("ddrl_dqn_eval", "trace_d"),
]


# ---- the stream contract's rows: the functions that take `void *stream` and no caller device memory ----------------------------------
# tests/test_gpu_abi_stream.py runs every case above AND these on a side stream (tests/_abi_arena.run_stream_case); the memory suite
# keeps CASES.  STREAM_TABLE() = TABLE + STREAM_ROWS is what tests/test_abi_table_cpu.py parses the header's stream parameters against.
# Each effect is read back into a declared output through the family's export entry; the *_h scalars are host outputs (ctx.host).
#
# A call that reads and writes handle memory only would, misplaced on another stream, simply finish during the gate: the setup settled
# that memory before the gate, and the read-back queued on `s` behind it finds what the twin finds.  So in every closure a call on `s`
# that does NOT COMMUTE with the call under test stands ahead of it (the "call ahead"): one that takes a declared input (a decoy until
# the late writes) and changes the handle state the call under test reads or writes — a store into the ring it draws from, a
# set_weights of the network it runs, a set_state of the env it reads, a winq_begin of the queue it reads — or a draw from the
# generator it reseeds.  The call ahead waits behind the gate; a call under test that ran during the gate acted on the state from
# before it, and the read-back differs from the twin's.
STREAM_EXEMPT = {
    "ddrl_comm_bcast_params": EXEMPT["ddrl_comm_bcast_params"],
    "ddrl_comm_allreduce_grads": EXEMPT["ddrl_comm_allreduce_grads"],
    "ddrl_comm_send_batch": EXEMPT["ddrl_comm_send_batch"],
    "ddrl_comm_recv_batch": EXEMPT["ddrl_comm_recv_batch"],
    "ddrl_dqn_step_timed": "profiling entry: it times the launches of ddrl_dqn_step, which has a row, between events and returns host means",
    "ddrl_sac1_stage_time": "profiling entry: it times one launch of ddrl_sac1_step, which has a row, between events and returns a host mean",
}
STREAM_CASES = {}   # id -> (fn, (functions covered))
STREAM_ROWS = {}    # function -> [case ids]


def stream_case(cid, *functions):
    def deco(fn):
        assert cid not in CASES and cid not in STREAM_CASES, cid
        STREAM_CASES[cid] = (fn, functions)
        for f in functions:
            STREAM_ROWS.setdefault(f, []).append(cid)
        return fn
    return deco


def STREAM_TABLE():
    t = {f: list(c) for f, c in TABLE.items()}
    for f, c in STREAM_ROWS.items():
        t.setdefault(f, []).extend(c)
    return t


def _at(arr, i=0):
    """Element i of a ctx.host array as the pointer the binding's prototype wants."""
    return ctypes.cast(ctypes.addressof(arr) + i * ctypes.sizeof(arr._type_), POINTER(arr._type_))


def _counts(ctx, name, h):
    c = ctx.host(name, 4, c_int64)
    return lambda: ctx.lib.ddrl_replay_counts(h, _at(c, 0), _at(c, 1), _at(c, 2), _at(c, 3), ctx.stream_arg)


def _copy_out(ctx, name, ptr, n_f32):
    """Closure part: n_f32 32-bit words of handle-owned device memory into output `name`, device to device on the current stream."""
    from distributed_drl_amd.replay import _view
    ctx.tensor(name).view(F32).copy_(_view(ptr, (n_f32,), ctx.device))


def _store_ahead(ctx, h, rows):
    """Call ahead: ddrl_replay_store of `rows` (obs1, acts, rews, obs2, done; declared inputs) on the caller's stream."""
    n = len(rows[2])
    p = [P(ctx.inp("ahead.%s" % k, x)) for k, x in zip(("obs_d", "act_d", "rew_d", "obs2_d", "done_d"), rows)]
    return lambda: ctx.lib.ddrl_replay_store(h, *p, n, ctx.stream_arg)


def _other_state(ctx, n, model, max_ep_len, discrete=False):
    """The state of a second env (another seed, one step taken), as the array that ddrl_env_set_state takes."""
    h2, fields = _env(ctx, n, model, seed=8, max_ep_len=max_ep_len)
    _env_warm(ctx, h2, n, discrete)
    src = ctx.tmp(torch.empty(fields * n, dtype=torch.float32))
    _ok(ctx, ctx.lib.ddrl_env_get_state(h2, _tp(src), None))
    ctx.sync()
    return src.cpu().numpy()


@stream_case("replay_seed", "ddrl_replay_seed")
def _seed(ctx):
    """Call ahead: a draw.  A seed that ran during the gate is followed by two draws, not one."""
    L = ctx.lib
    h = _ring5(ctx, 8, 2, fill=37)
    idx0, idx = ctx.out("idx0_d", 37, I64), ctx.out("idx_d", 37, I64)
    return lambda: [L.ddrl_replay_sample_indices(h, 37, P(idx0), ctx.stream_arg), L.ddrl_replay_seed(h, 99, ctx.stream_arg),
                    L.ddrl_replay_sample_indices(h, 37, P(idx), ctx.stream_arg)]


@stream_case("replay_counts-behind_masked_store", "ddrl_replay_counts")
def _counts_masked(ctx):
    """The masked store's row count stays on the device: counts reads it behind a sync of `stream`, on which the store still waits."""
    L, (Ln, obs), n = ctx.lib, WINDOWS["Ln3o5"], 37
    h = _wring(ctx, Ln, obs, fill=7)
    src = _ptrs(*[ctx.inp("src_h[%d]" % j, x) for j, x in enumerate(_wrows(Ln, obs, n, 5))])
    md = ctx.inp("mask_d", (np.arange(n) % 3 == 0).astype(np.uint8))
    cnt = _counts(ctx, "counts_h", h)
    exp = _export5(ctx, h, _wwidths(Ln, obs), CAP)
    return lambda: [L.ddrl_replay_store_masked_ex(h, src, P(md), n, ctx.stream_arg), cnt()] + exp()


@stream_case("replay_set_counts", "ddrl_replay_set_counts", "ddrl_replay_counts")
def _set_counts(ctx):
    """Call ahead: a store of three rows.  Counters set during the gate are moved on by the store."""
    L = ctx.lib
    h = _ring5(ctx, 8, 2, fill=37)
    ahead = _store_ahead(ctx, h, _rows5(8, 2, 3, 9, 0))
    idx = ctx.out("idx_d", 16, I64)
    cnt = _counts(ctx, "counts_h", h)
    return lambda: [ahead(), L.ddrl_replay_set_counts(h, 5, 20, 100, 7, ctx.stream_arg),
                    L.ddrl_replay_sample_indices(h, 16, P(idx), ctx.stream_arg), cnt()]


@stream_case("replay_mt_state", "ddrl_replay_mt_state")
def _mt_state(ctx):
    L = ctx.lib
    h = _ring5(ctx, 8, 2, fill=37)
    idx = ctx.out("idx_d", 37, I64)
    key, pos = ctx.host("key_h", 624, c_uint32), ctx.host("pos_h", 1, c_int32)
    return lambda: [L.ddrl_replay_sample_indices(h, 37, P(idx), ctx.stream_arg), L.ddrl_replay_mt_state(h, key, _at(pos), ctx.stream_arg)]


@stream_case("replay_append_ring", "ddrl_replay_append_ring")
def _append_ring(ctx):
    """45 rows in a ring of 50 take 13 more: the append wraps; the staging ring is emptied (its counts are host outputs).
    Call ahead: the store of the staging ring's last three rows.  An append that ran during the gate moved ten rows and left three."""
    L = ctx.lib
    dst, src = _ring5(ctx, 8, 2, fill=45), _ring5(ctx, 8, 2, cap=16, fill=10, seed=4)
    ahead = _store_ahead(ctx, src, _rows5(8, 2, 3, 9, 0))
    exp = _export5(ctx, dst, (8, 8, 2, 1, 1), CAP)
    cd, cs = _counts(ctx, "dst.counts_h", dst), _counts(ctx, "src.counts_h", src)
    return lambda: [ahead(), L.ddrl_replay_append_ring(dst, src, ctx.stream_arg)] + exp() + [cd(), cs()]


LSHAPE = "o8a2h64x48B37"     # SAC_SHAPES' direct-operand one


def _sac_ring(ctx, cap=CAP, fill=37):
    return _ring5(ctx, 8, 2, cap=cap, fill=fill)


def _sac_sets(ctx, h):
    L, sets = ctx.lib, []
    for s in (0, 1):
        b = (P * 8)()
        _ok(ctx, L.ddrl_sac1_input_buffers(h, s, b))
        sets.append([int(b[i]) for i in range(8)])
    return sets


def _mk_sac_two_phase(variant):
    def fn(ctx):
        L = ctx.lib
        h, n = _sac(ctx, LSHAPE, variant)
        ins = [P(ctx.inp(k, x)) for k, x in _sac_batch(LSHAPE, 31)]
        losses = P(ctx.out("losses_d", 4 if variant else 3, F32))
        exp = [(w, P(ctx.out("export%d" % w, n, F32))) for w in (0, 1, 2, 3)]
        s = lambda: ctx.stream_arg
        return lambda: [L.ddrl_sac1_compute_grads(h, *ins, losses, None, None, None, s()), L.ddrl_sac1_grad_finalize(h, s()),
                        L.ddrl_sac1_apply_grads(h, s())] + [L.ddrl_sac1_export(h, w, p, s()) for w, p in exp]
    return fn


stream_case("sac1_grad_finalize_apply_grads", "ddrl_sac1_grad_finalize", "ddrl_sac1_apply_grads")(_mk_sac_two_phase(0))
stream_case("sacv_grad_finalize_apply_grads", "ddrl_sac1_grad_finalize", "ddrl_sac1_apply_grads")(_mk_sac_two_phase(1))


@stream_case("sac1_opt_state_set_get_steps", "ddrl_sac1_opt_state_set", "ddrl_sac1_opt_state_get", "ddrl_sac1_opt_steps")
def _opt_state(ctx):
    """One update (the call ahead: it takes the batch and moves the counts) -> set(3, 4, ctr) -> one update (its lr_t depends on the
    counts) -> the counts read back both ways, behind the update.  A set that ran during the gate is counted on by two updates."""
    L = ctx.lib
    h, n = _sac(ctx, LSHAPE)
    ins = [P(ctx.inp(k, x)) for k, x in _sac_batch(LSHAPE, 31)]
    losses = P(ctx.out("losses_d", 3, F32))
    e0 = P(ctx.out("export0", n, F32))
    t, g, c = ctx.host("opt_steps_h", 2, c_int64), ctx.host("opt_state_h", 2, c_int64), ctx.host("noise_ctr_h", 1, c_uint64)
    s = lambda: ctx.stream_arg
    return lambda: [L.ddrl_sac1_step(h, *ins, losses, None, None, None, s()),
                    L.ddrl_sac1_opt_state_set(h, 3, 4, 1234, s()), L.ddrl_sac1_step(h, *ins, losses, None, None, None, s()),
                    L.ddrl_sac1_export(h, 0, e0, s()), L.ddrl_sac1_opt_steps(h, _at(t, 0), _at(t, 1), s()),
                    L.ddrl_sac1_opt_state_get(h, _at(g, 0), _at(g, 1), _at(c), s())]


def _mk_sac_and_sample(mode):
    """The learner's own input sets: set 0 holds a drawn batch (setup), the call under test updates from it while its sampler draws
    the next batch into set 1; both sets' transition arrays and the generated noise of set 0 are copied out.
    Calls ahead: a set_weights of the learner and a store of three rows into the ring the sampler draws from (ddrl_sac1_fill_noise
    launches nothing: it arms the next update's first kernel)."""
    o, a, _, _, B = SAC_SHAPES[LSHAPE]

    def fn(ctx):
        L = ctx.lib
        h, n = _sac(ctx, LSHAPE)
        ring = _sac_ring(ctx)
        sets = _sac_sets(ctx, h)
        _ok(ctx, L.ddrl_replay_sample(ring, B, *[P(x) for x in sets[0][:5]], None, None))
        flat, store = P(ctx.inp("ahead.flat_d", _weights(n, 23))), _store_ahead(ctx, ring, _rows5(8, 2, 3, 9, 0))
        # (the two fused entries take no losses pointer: the loss words stay in the handle)
        losses = P(ctx.out("losses_d", 3, F32)) if mode == "apply_grads_and_sample" else None
        exp =[(w, P(ctx.out("export%d" % w, n, F32))) for w in (0, 2)]
        widths = (o, o, a, 1, 1, a, a, a)
        for k in (0, 1):
            for j in range(8 if k == 0 else 5):
                ctx.out("set%d[%d]" % (k, j), B * widths[j], F32)
        s = lambda: ctx.stream_arg

        def call():
            ahead = [L.ddrl_sac1_set_weights(h, flat, s()), store()]
            if mode == "step_and_sample":
                rc = [L.ddrl_sac1_fill_noise(h, 11, s()), L.ddrl_sac1_step_and_sample(h, 0, ring, 1, s())]
            elif mode == "compute_grads_and_sample":
                rc = [L.ddrl_sac1_fill_noise(h, 11, s()), L.ddrl_sac1_compute_grads_and_sample(h, 0, ring, 1, s()),
                      L.ddrl_sac1_grad_finalize(h, s()), L.ddrl_sac1_apply_grads(h, s())]
            else:
                rc = [L.ddrl_sac1_fill_noise(h, 11, s()),
                      L.ddrl_sac1_compute_grads(h, *[P(x) for x in sets[0]], losses, None, None, None, s()),
                      L.ddrl_sac1_apply_grads_and_sample(h, ring, 1, s())]
            rc = ahead + rc + [L.ddrl_sac1_export(h, w, p, s()) for w, p in exp]
            for k in (0, 1):
                for j in range(8 if k == 0 else 5):
                    _copy_out(ctx, "set%d[%d]" % (k, j), sets[k][j], B * widths[j])
            return rc
        return call
    return fn


for _m, _f in (("step_and_sample", ("ddrl_sac1_step_and_sample", "ddrl_sac1_fill_noise")),
               ("compute_grads_and_sample", ("ddrl_sac1_compute_grads_and_sample", "ddrl_sac1_fill_noise")),
               ("apply_grads_and_sample", ("ddrl_sac1_apply_grads_and_sample", "ddrl_sac1_fill_noise"))):
    stream_case("sac1_%s" % _m, *_f)(_mk_sac_and_sample(_m))


@stream_case("sac1_graph_sync", "ddrl_sac1_graph_sync")
def _graph_sync(ctx):
    """One update leaves the double-buffered optimizer state on copy 1; graph_sync puts it back on copy 0 (a copy node on `stream`);
    the update behind it continues from there."""
    L = ctx.lib
    h, n = _sac(ctx, LSHAPE)
    ins = [P(ctx.inp(k, x)) for k, x in _sac_batch(LSHAPE, 31)]
    losses = P(ctx.out("losses_d", 3, F32))
    exp = [(w, P(ctx.out("export%d" % w, n, F32))) for w in (0, 1, 2, 3)]
    s = lambda: ctx.stream_arg
    return lambda: [L.ddrl_sac1_step(h, *ins, losses, None, None, None, s()), L.ddrl_sac1_graph_sync(h, s()),
                    L.ddrl_sac1_step(h, *ins, losses, None, None, None, s())] + [L.ddrl_sac1_export(h, w, p, s()) for w, p in exp]


LOOP_ROWS = 64


def _mk_loop_run(per_graph):
    """Two calls: per_graph - 1 updates (below the capture threshold: eager), then 2 per_graph + 1 (one eager update, the capture, replays).
    Calls ahead: a set_weights of the learner and a store of three rows into the ring the loop draws from."""
    def fn(ctx):
        L = ctx.lib
        h, n = _sac(ctx, LSHAPE)
        ring = _sac_ring(ctx, cap=LOOP_ROWS, fill=LOOP_ROWS)
        flat, store = P(ctx.inp("ahead.flat_d", _weights(n, 23))), _store_ahead(ctx, ring, _rows5(8, 2, 3, 9, 0))
        loop = _handle(ctx, L.ddrl_loop_destroy, L.ddrl_loop_create, h, ring, per_graph, 13)
        exp = [(w, P(ctx.out("export%d" % w, n, F32))) for w in (0, 1, 2, 3)]
        t = ctx.host("opt_steps_h", 2, c_int64)
        cnt = _counts(ctx, "counts_h", ring)
        s = lambda: ctx.stream_arg
        return lambda: [L.ddrl_sac1_set_weights(h, flat, s()), store(), L.ddrl_loop_run(loop, per_graph - 1, s()),
                        L.ddrl_loop_run(loop, 2 * per_graph + 1, s())] + [
            L.ddrl_sac1_export(h, w, p, s()) for w, p in exp] + [L.ddrl_sac1_opt_steps(h, _at(t, 0), _at(t, 1), s()), cnt()]
    return fn


def _mk_dqn_loop_run(per_graph):
    shape = "o8A2h64x48B37"
    o, A, _, _, B = DQN_SHAPES[shape]

    def fn(ctx):
        L = ctx.lib
        h, n, _ = _dqn(ctx, shape, 0)
        ring = _ring5(ctx, o, 1, 0, cap=LOOP_ROWS, fill=0)
        r = _rs(72)
        rows = [_f32(r.randn(LOOP_ROWS, o)), _f32(r.randint(0, A, (LOOP_ROWS, 1))), _f32(r.randn(LOOP_ROWS)), _f32(r.randn(LOOP_ROWS, o)),
                _f32(r.rand(LOOP_ROWS) < 0.2)]
        _ok(ctx, L.ddrl_replay_store(ring, *[_tp(ctx.tmp(x)) for x in rows], LOOP_ROWS, None))
        flat = P(ctx.inp("ahead.flat_d", _weights(n, 57) * 0.25))
        store = _store_ahead(ctx, ring, [_f32(r.randn(3, o)), _f32(r.randint(0, A, (3, 1))), _f32(r.randn(3)), _f32(r.randn(3, o)),
                                         _f32(r.rand(3) < 0.2)])
        ld = P(ctx.out("loss_d", 1, F32))
        loop = _handle(ctx, L.ddrl_dqn_loop_destroy, L.ddrl_dqn_loop_create, h, ring, per_graph, ld)
        exp = [(w, P(ctx.out("export%d" % w, n, F32))) for w in (0, 1, 2, 3)]
        cnt = _counts(ctx, "counts_h", ring)
        s = lambda: ctx.stream_arg
        return lambda: [L.ddrl_dqn_set_weights(h, flat, s()), store(), L.ddrl_dqn_loop_run(loop, per_graph - 1, s()),
                        L.ddrl_dqn_loop_run(loop, 2 * per_graph + 1, s())] + [
            L.ddrl_dqn_export(h, w, p, s()) for w, p in exp] + [cnt()]
    return fn


for _pg in (2, 3):
    stream_case("loop_run-per_graph%d" % _pg, "ddrl_loop_run")(_mk_loop_run(_pg))
    stream_case("dqn_loop_run-per_graph%d" % _pg, "ddrl_dqn_loop_run")(_mk_dqn_loop_run(_pg))


@stream_case("actor_versions_enable", "ddrl_actor_versions_enable")
def _actor_enable(ctx):
    """A set_weights (the call ahead: what enable keeps as the first version) -> enable -> a second install -> three envs adopt it:
    the slot words and the action of every env against its version."""
    L = ctx.lib
    h, n_pi = _actor(ctx)
    src0 = P(ctx.inp("ahead.flat_pi_d", _weights(n_pi, 44)))
    src = P(ctx.inp("flat_pi_d", _weights(n_pi, 43)))
    ended = np.zeros(MAX_ROWS, np.uint8)
    ended[[0, 3, 40]] = 1
    e = P(ctx.inp("ended_d", ended))
    r = _rs(6)
    obs, eps = P(ctx.inp("obs_d", _f32(r.randn(MAX_ROWS, 8)))), P(ctx.inp("eps_d", _f32(r.randn(MAX_ROWS, 2))))
    slots, act = P(ctx.out("slot_of_env_d", MAX_ROWS, I32)), P(ctx.out("act_d", MAX_ROWS * 2, F32))
    st = ctx.host("state_h", 4, c_int32)
    s = lambda: ctx.stream_arg
    return lambda: [L.ddrl_actor_set_weights(h, src0, s()), L.ddrl_actor_versions_enable(h, 8, s()), L.ddrl_actor_set_weights(h, src, s()),
                    L.ddrl_actor_versions_adopt(h, e, MAX_ROWS, s()), L.ddrl_actor_act_versioned(h, obs, eps, MAX_ROWS, 0, 1000, act, s()),
                    L.ddrl_actor_versions_state(h, slots, st, s())]


@stream_case("dqn_versions_enable", "ddrl_dqn_versions_enable")
def _dqn_enable(ctx):
    """_actor_enable's on the Q network; the Q values of every env against its version come out of one fused rollout step (the only
    versioned forward of this family)."""
    L = ctx.lib
    h, n, _ = _dqn(ctx, DSHAPE)
    env, _ = _env(ctx, RN, "one_body", max_ep_len=3)
    ring = _ring5(ctx, 8, 1, cap=RCAP, fill=7)
    src0 = P(ctx.inp("ahead.flat_main_d", _weights(n, 54) * 0.25))
    src = P(ctx.inp("flat_main_d", _weights(n, 53) * 0.25))
    ended = np.zeros(RN, np.uint8)
    ended[[0, 3, 40]] = 1
    e = P(ctx.inp("ended_d", ended))
    slots = P(ctx.out("slot_of_env_d", RN, I32))
    am, qm = P(ctx.out("act_out_d", RN, F32)), P(ctx.out("q_out_d", RN * 4, F32))
    st = ctx.host("state_h", 4, c_int32)
    s = lambda: ctx.stream_arg
    return lambda: [L.ddrl_dqn_set_weights(h, src0, s()), L.ddrl_dqn_versions_enable(h, 8, s()), L.ddrl_dqn_set_weights(h, src, s()),
                    L.ddrl_dqn_versions_adopt(h, e, RN, s()), L.ddrl_rollout_begin_discrete(env, h, s()),
                    L.ddrl_rollout_step_discrete(env, h, ring, 1, 0, 0.5, 5, 1000, am, qm, None, s()),
                    L.ddrl_dqn_versions_state(h, slots, st, s())]


def _mk_rollout_begin(model):
    """Two fused steps, then a step outside the fused path: the actor's rows are stale, the begin call under test refreshes them and
    the fused step behind it acts on what it copied.  Call ahead: a set_state with the state of another env; a begin that ran during
    the gate copied the observations of the state before it."""
    def fn(ctx):
        L = ctx.lib
        h, fields = _env(ctx, RN, model, max_ep_len=3)
        ahead = P(ctx.inp("ahead.state_d", _other_state(ctx, RN, model, 3)))
        a, _ = _actor(ctx)
        ring = _ring5(ctx, 8, 2, cap=RCAP, fill=7)
        begin, step = ((L.ddrl_rollout_begin_articulated, L.ddrl_rollout_step_articulated) if model == "articulated"
                       else (L.ddrl_rollout_begin, L.ddrl_rollout_step))
        _ok(ctx, begin(h, a, None))
        _ok(ctx, step(h, a, ring, 2, 5, 0, 0, None, None, None))
        _env_warm(ctx, h, RN)
        am, om = P(ctx.out("act_out_d", RN * 2, F32)), P(ctx.out("next_obs_out_d", RN * 8, F32))
        st = P(ctx.out("state_d", fields * RN, F32))
        exp = _export5(ctx, ring, (8, 8, 2, 1, 1), RCAP)
        s = lambda: ctx.stream_arg
        return lambda: [L.ddrl_env_set_state(h, ahead, s()), begin(h, a, s()), step(h, a, ring, 1, 5, 1000, 0, am, om, s()),
                        L.ddrl_env_get_state(h, st, s())] + exp()
    return fn


stream_case("rollout_begin", "ddrl_rollout_begin")(_mk_rollout_begin("one_body"))
stream_case("rollout_begin_articulated", "ddrl_rollout_begin_articulated")(_mk_rollout_begin("articulated"))


def _mk_rollout_begin_discrete(model):
    """The discrete pair likewise, the set_state ahead included.  The articulated pair takes handles only: its mirrors live in the env
    handle and are copied out."""
    artic = model == "articulated"

    def fn(ctx):
        L = ctx.lib
        h, fields = _env(ctx, RN, model, max_ep_len=3)
        ahead = P(ctx.inp("ahead.state_d", _other_state(ctx, RN, model, 3, discrete=True)))
        d, _, _ = _dqn(ctx, DSHAPE)
        ring = _ring5(ctx, 8, 1, cap=RCAP, fill=7)
        s = lambda: ctx.stream_arg
        st = P(ctx.out("state_d", fields * RN, F32))
        if artic:
            begin, step = L.ddrl_rollout_begin_discrete_articulated, L.ddrl_rollout_step_discrete_articulated
            _ok(ctx, begin(h, d, None))
            _ok(ctx, step(h, d, ring, 2, 0, 0.5, 5, 0, None))
            mir = [P(), P(), P()]
            _ok(ctx, L.ddrl_env_rollout_mirrors(h, byref(mir[0]), byref(mir[1]), byref(mir[2]), None, None))
            sizes = (("act_mirror", RN), ("q_mirror", RN * 4), ("next_obs_mirror", RN * 8))
            for k, w in sizes:
                ctx.out(k, w, F32)
        else:
            begin, step = L.ddrl_rollout_begin_discrete, L.ddrl_rollout_step_discrete
            _ok(ctx, begin(h, d, None))
            _ok(ctx, step(h, d, ring, 2, 0, 0.5, 5, 0, None, None, None, None))
            am, qm, om = P(ctx.out("act_out_d", RN, F32)), P(ctx.out("q_out_d", RN * 4, F32)), P(ctx.out("next_obs_out_d", RN * 8, F32))
        _env_warm(ctx, h, RN, discrete=True)
        exp = _export5(ctx, ring, (8, 8, 1, 1, 1), RCAP)

        def call():
            if artic:
                rc = [L.ddrl_env_set_state(h, ahead, s()), begin(h, d, s()), step(h, d, ring, 1, 0, 0.5, 5, 1000, s()),
                      L.ddrl_env_get_state(h, st, s())] + exp()
                for (k, w), p in zip(sizes, mir):
                    _copy_out(ctx, k, p.value, w)
                return rc
            return [L.ddrl_env_set_state(h, ahead, s()), begin(h, d, s()), step(h, d, ring, 1, 0, 0.5, 5, 1000, am, qm, om, s()),
                    L.ddrl_env_get_state(h, st, s())] + exp()
        return call
    return fn


stream_case("rollout_begin_discrete", "ddrl_rollout_begin_discrete")(_mk_rollout_begin_discrete("one_body"))
stream_case("rollout_discrete_articulated", "ddrl_rollout_begin_discrete_articulated",
            "ddrl_rollout_step_discrete_articulated")(_mk_rollout_begin_discrete("articulated"))


def _mk_rollout_begin_nstep(model):
    """_mk_rollout_nstep's setup, then reset + winq_begin outside the fused path: the actor's rows and the readiness bytes are stale and
    the begin call under test rebuilds them; the fused step behind it shows what it wrote.  Call ahead: a winq_begin with other
    observations (the begin launch reads the queues only); a begin that ran during the gate copied the rows from before it."""
    Ln, artic = 4, model == "articulated"

    def fn(ctx):
        from distributed_drl_amd import _lib
        L = ctx.lib
        h, fields = _env(ctx, RN, model, max_ep_len=1 << 20)
        a, _ = _actor(ctx)
        ring = _wring(ctx, Ln, 8, cap=RCAP)
        q = _handle(ctx, L.ddrl_winq_destroy, L.ddrl_winq_create, _dev(ctx), RN, Ln, 8, 2, 1)
        begin, step = ((L.ddrl_rollout_begin_nstep_articulated, L.ddrl_rollout_step_nstep_articulated) if artic
                       else (L.ddrl_rollout_begin_nstep, L.ddrl_rollout_step_nstep))
        obs = ctx.tmp(torch.empty(RN * 8, dtype=torch.float32))
        args = (0.3, 0.1, 5.0, 2, 3, 0, 5)
        _ok(ctx, L.ddrl_env_reset(h, None, _tp(obs), None))
        _ok(ctx, L.ddrl_winq_begin(q, None, _tp(obs), None))
        _ok(ctx, begin(h, a, q, None))
        _ok(ctx, step(h, a, q, ring, 4, *args, 0, None, None))
        _ok(ctx, L.ddrl_env_reset(h, None, _tp(obs), None))
        _ok(ctx, L.ddrl_winq_begin(q, None, _tp(obs), None))
        ahead = P(ctx.inp("ahead.obs_d", _f32(_rs(12).randn(RN, 8))))
        names = (("act", 2, F32), ("obs2", 8, F32), ("rew", 1, F32), ("done", 1, F32), ("next_obs", 8, F32), ("ended", 1, U8))
        out = ctx.keep(_lib.RolloutNStepOut(*[P(ctx.out("out->" + k, RN * w, t)) for k, w, t in names]))
        st = P(ctx.out("state_d", fields * RN, F32))
        exp = _export5(ctx, ring, _wwidths(Ln, 8), RCAP)
        s = lambda: ctx.stream_arg
        return lambda: [L.ddrl_winq_begin(q, None, ahead, s()), begin(h, a, q, s()), step(h, a, q, ring, 1, *args, 4000, byref(out), s()),
                        L.ddrl_env_get_state(h, st, s())] + exp()
    return fn


stream_case("rollout_begin_nstep", "ddrl_rollout_begin_nstep")(_mk_rollout_begin_nstep("one_body"))
stream_case("rollout_begin_nstep_articulated", "ddrl_rollout_begin_nstep_articulated")(_mk_rollout_begin_nstep("articulated"))


def _mk_env_stats(model):
    """max_ep_len 2 and one step taken: the step under test ends every episode at the limit; the statistics are read behind it."""
    n = 33

    def fn(ctx):
        L = ctx.lib
        h, _ = _env(ctx, n, model)
        _env_warm(ctx, h, n)
        act = P(ctx.inp("act_d", _f32(_rs(2).uniform(-1.2, 1.2, (n, 2)))))
        rew = P(ctx.out("rew_d", n, F32))
        ep, ret, ln = ctx.host("episodes_h", 1, c_int64), ctx.host("ret_sum_h", 1, c_double), ctx.host("len_sum_h", 1, c_int64)
        s = lambda: ctx.stream_arg
        return lambda: [L.ddrl_env_step(h, act, None, rew, None, None, None, s()), L.ddrl_env_stats(h, _at(ep), _at(ret), _at(ln), s())]
    return fn


for _m in MODELS:
    stream_case("env_stats-%s" % _m, "ddrl_env_stats")(_mk_env_stats(_m))


def _mk_env_eval(model, discrete):
    """The evaluation entries fed from handles: the results live in a block of the env handle (ddrl_env_eval_results) and are copied
    out.  A first evaluation of the same size (setup) has allocated that block, so that the call under test only launches.
    Call ahead: a set_weights of the network that the episodes are played with."""
    row = 20 if discrete else 12

    def fn(ctx):
        L = ctx.lib
        h, _ = _env(ctx, 1, model, seed=5, max_ep_len=EP_LEN)
        src, n, _ = _dqn(ctx, DSHAPE) if discrete else _actor(ctx) + (None,)
        flat = P(ctx.inp("ahead.flat_d", _weights(n, 58) * (0.25 if discrete else 1.0)))
        setw = L.ddrl_dqn_set_weights if discrete else L.ddrl_actor_set_weights
        s = lambda: ctx.stream_arg
        if discrete:
            ev = lambda first, st: L.ddrl_env_eval_q(h, src, EPISODES, first, 0, 0.5, 9, 100, 1, st)
        else:
            ev = lambda first, st: L.ddrl_env_eval_policy(h, src, EPISODES, first, 1, st)
        _ok(ctx, ev(0, None))
        ctx.out("ret", EPISODES, F64), ctx.out("len", EPISODES, I32), ctx.out("trace", EPISODES * EP_LEN * row, F32)

        def call():
            rc = [setw(src, flat, s()), ev(2, s())]
            ret, ln, tr = P(), P(), P()
            ne, ml, tw = c_int32(), c_int32(), c_int32()
            _ok(ctx, L.ddrl_env_eval_results(h, byref(ret), byref(ln), byref(tr), byref(ne), byref(ml), byref(tw)))
            assert (ne.value, ml.value, tw.value) == (EPISODES, EP_LEN, row), (ne.value, ml.value, tw.value)
            _copy_out(ctx, "ret", ret.value, 2 * EPISODES)
            _copy_out(ctx, "len", ln.value, EPISODES)
            _copy_out(ctx, "trace", tr.value, EPISODES * EP_LEN * row)
            return rc
        return call
    return fn


for _m in MODELS:
    stream_case("env_eval_policy-%s" % _m, "ddrl_env_eval_policy")(_mk_env_eval(_m, False))
    stream_case("env_eval_q-%s" % _m, "ddrl_env_eval_q")(_mk_env_eval(_m, True))
