"""ddrl_replay_append_ring / _Ring.append_from: commit a staging ring whose fill count lives on the device.

REFERENCE  a twin of the destination ring that receives the same rows, oldest first, through store_batch — `size` sequential store()
calls, which is what the append is defined to equal.  Every comparison is bit-exact and covers the WHOLE destination ring (the rows the
append must not touch included), its counters, and the source: emptied (ptr = size = 0), everything else of it untouched."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

KINDS = ("sac", "dqn", "nstep")
LN = 3
SRC_CAP = 96


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _make(ddrl, kind, cap, seed=None, **kw):
    if kind == "sac":
        return ddrl.ReplayBuffer(8, 2, cap, seed=seed, **kw)
    if kind == "dqn":
        return ddrl.ReplayBufferDQN(type("Opt", (), dict(obs_dim=8, buffer_size=cap, batch_size=4))(), 0, seed=seed, **kw)
    opt = type("Opt", (), dict(Ln=LN, obs_shape=(8,), act_shape=(2,), buffer_size=cap, num_buffers=2, batch_size=4))()
    return ddrl.ReplayBufferNStep(opt, seed=seed)       # num_buffers = 2: the counters advance by two per row


def _data(kind, n, seed):
    """n seeded rows, as host arrays in the ring's store_batch argument order."""
    rs = np.random.RandomState(seed)
    f = lambda *s: rs.randn(*s).astype(np.float32)
    if kind == "nstep":
        return [f(n, LN + 1, 8), f(n, LN, 2), f(n, LN), (rs.rand(n, LN) < 0.2).astype(np.float32)]
    act = rs.randint(0, 4, n).astype(np.float32) if kind == "dqn" else f(n, 2)
    return [f(n, 8), act, f(n), f(n, 8), (rs.rand(n) < 0.2).astype(np.float32)]     # obs, act, rew, next_obs, done


def _store(ring, data, lo=0, hi=None):
    rows = [x[lo:hi] for x in data]
    if rows[0].shape[0]:
        ring.store_batch(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in rows))


def _arrays(ring):
    return {k: v.clone() for k, v in ring.rings().items()}


def _same_ring(got, want, what):
    a, b = _arrays(got), _arrays(want)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: array %s differs" % (what, k)
    assert got._counts() == want._counts(), "%s: (ptr, size, steps, sample_times) %r, twin %r" % (what, got._counts(), want._counts())


def _destinations(ddrl, kind):
    """(name, ring, twin): A — capacity 100 with 90 seeded rows, so the append wraps; B — capacity 50 < 96: the skip rule."""
    out = []
    for name, cap, pre in (("A", 100, 90), ("B", 50, 7)):
        pair = [_make(ddrl, kind, cap, seed=3) for _ in range(2)]
        for r in pair:
            _store(r, _data(kind, pre, 50 + cap))
        out.append((name, pair[0], pair[1]))
    return out


def _filled_source(ddrl, kind, stored):
    """A source of capacity 96 after `stored` store() calls of seeded rows and one draw; (ring, data, first row it still holds)."""
    src = _make(ddrl, kind, SRC_CAP, seed=7)
    data = _data(kind, stored, 1000 + stored)
    _store(src, data)
    if stored:
        src.sample_batch_device(4)      # sample_times and the MT19937 position move: the append must leave both alone
    return src, data, max(0, stored - SRC_CAP)


# ---- 1. append == sequential stores --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stored", [0, 1, 37, 96, 130])
@pytest.mark.parametrize("kind", KINDS)
def test_append_equals_sequential_stores(ddrl, kind, stored):
    """c in {0, 1, 37, 96} rows in an unwrapped source, and 130 rows stored into capacity 96 (wrapped: it holds rows 34 .. 129, the oldest
    at its cursor).  Widths 8 / 8 / 2 / 1 / 1 and 32 / 6 / 3 / 3: the float4 and the scalar path, and a 1-D action array."""
    for name, dst, twin in _destinations(ddrl, kind):
        src, data, first = _filled_source(ddrl, kind, stored)
        before = (_arrays(src), src._counts(), src.mt_state())
        dst.append_from(src)
        _store(twin, data, first, stored)
        what = "%s, %d stored, destination %s" % (kind, stored, name)
        _same_ring(dst, twin, what)
        ptr, size, steps, samples = src._counts()
        assert (ptr, size) == (0, 0), what
        assert (steps, samples) == before[1][2:], what
        key, pos = src.mt_state()
        assert pos == before[2][1] and np.array_equal(key, before[2][0]), what
        after = _arrays(src)
        for k in after:
            assert torch.equal(after[k], before[0][k]), "%s: source array %s changed" % (what, k)
        # the emptied source takes rows again from row 0, and a second append commits exactly those
        more = _data(kind, 5, 77)
        _store(src, more)
        dst.append_from(src)
        _store(twin, more)
        _same_ring(dst, twin, what + ", second append")


# ---- 2. a count the host never learns ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", ["half", "none"])
def test_append_after_masked_stores_reads_the_count_on_the_device(ddrl, mask_kind):
    """The source is filled through store_masked (64 candidate rows, a seeded mask with about half set; and an all-zero mask): how many
    rows it holds is in its device state only — no get_counts() between the store and the append."""
    n = 64
    data = _data("nstep", n, 9)
    mask = (np.random.RandomState(4).rand(n) < 0.5) if mask_kind == "half" else np.zeros(n, bool)
    assert (0 < mask.sum() < n) if mask_kind == "half" else mask.sum() == 0
    for name, dst, twin in _destinations(ddrl, "nstep"):
        src = _make(ddrl, "nstep", SRC_CAP, seed=7)
        src.store_masked(*(torch.from_numpy(x).cuda() for x in data), torch.from_numpy(mask.astype(np.uint8)).cuda())
        dst.append_from(src)
        _store(twin, [x[mask] for x in data])
        _same_ring(dst, twin, "masked (%s), destination %s" % (mask_kind, name))
        assert src._counts()[:2] == (0, 0)


# ---- 3. one captured node follows the counts at replay -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sac", "nstep"])
def test_a_captured_append_follows_the_counts_at_replay(ddrl, kind):
    """One append_from captured in a (linear) graph; replayed with 5 rows in the source, then with 41: equals two eager appends."""
    data = _data(kind, 46, 21)
    (_, dst, twin), _ = _destinations(ddrl, kind)
    src, src2 = _make(ddrl, kind, SRC_CAP), _make(ddrl, kind, SRC_CAP)
    dst.append_from(src)                 # an empty source: a no-op (and the kernel is loaded before the capture)
    _same_ring(dst, twin, "%s: empty source" % kind)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dst.append_from(src)
    for lo, hi in ((0, 5), (5, 46)):
        _store(src, data, lo, hi)
        _store(src2, data, lo, hi)
        torch.cuda.synchronize()         # the stores above ran on the caller's stream, the replay has its own
        g.replay()
        torch.cuda.synchronize()
        twin.append_from(src2)
        _same_ring(dst, twin, "%s: replay with rows %d..%d" % (kind, lo, hi))
        assert src._counts()[:2] == (0, 0)
    assert dst._counts()[2] == twin._counts()[2] > 0


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_change_neither_ring(ddrl):
    from distributed_drl_amd._lib import DdrlUnsupported
    rows = _data("sac", 10, 1)
    # integer-valued observations in [0, 255]: what a compact ring holds
    pix = [np.minimum(np.floor(np.abs(x) * 40), 255).astype(np.float32) if x.ndim == 2 and x.shape[1] == 8 else x for x in rows]

    def ring(obs=8, compact=False):
        r = ddrl.ReplayBuffer(obs, 2, 32, seed=1, compact_obs=compact)
        _store(r, [x[:, :obs] if (x.ndim == 2 and x.shape[1] == 8) else x for x in pix])
        return r

    nst = _make(ddrl, "nstep", 32)
    _store(nst, _data("nstep", 10, 2))
    cases = {"widths": (ring(), ring(obs=6)), "n_arrays": (ring(), nst), "compact destination": (ring(compact=True), ring()),
             "compact source": (ring(), ring(compact=True))}
    same = ring()
    cases["dst is src"] = (same, same)
    for what, (dst, src) in cases.items():
        before = [(_arrays(r), r._counts()) for r in (dst, src)]
        with pytest.raises((DdrlUnsupported, ValueError)) as e:
            dst.append_from(src)
        assert "ddrl_replay_append_ring" in str(e.value), what
        for r, (arrs, counts) in zip((dst, src), before):
            assert r._counts() == counts, what
            now = _arrays(r)
            for k in arrs:
                assert torch.equal(now[k], arrs[k]), (what, k)
