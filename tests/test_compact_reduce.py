"""The kernels behind multiview.compact_allreduce (csrc/compact.hip; needs an MI355X: -m gpu):
visibility_pack against numpy's packing of count > 0, union_plan against numpy.flatnonzero of the
OR of the ranks' words, rows_gather / rows_scatter against index_select, bitwise.  Single process,
no collective.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SIZES = [1, 31, 32, 33, 63, 64, 65, 1000, 4099]
FILL = 0x7fc00abc  # a NaN pattern nothing computes: an element still holding it was not written
SENTINEL = -12345


def _C():
    from diff_gaussian_rasterization import _C
    return _C


def _rpw():
    return _C().union_rows_per_wave()


def _large_sizes():
    """union_offsets_kernel: 256 threads, thread t owns the per = ceil(nw / 256) waves from t per on.
    256 waves (every thread one: the serial pass sees 256 partial sums), 257 waves (per = 2: threads
    0..127 two waves, thread 128 the last wave of one row) and 770 waves less 19 rows (per = 4)."""
    rpw = _rpw()
    return [256 * rpw, 256 * rpw + 1, 770 * rpw - 19]


def _plan_sizes():
    return SIZES + [2 * _rpw() + 5, 5 * _rpw()] + _large_sizes()


def _plan_bounds(P, rpw):
    """Every wave boundary and P; beyond 16 of them: the first waves of threads 0 and 1 at per = 2,
    a thread's second wave (3 rpw: that offset is written inside the thread's own loop, not taken from
    the partial sums), the waves around 256, the last wave and P."""
    bounds = list(range(0, P, rpw)) + [P]
    if len(bounds) > 16:
        nw = (P + rpw - 1) // rpw
        bounds = sorted({0, rpw, 2 * rpw, 3 * rpw, 255 * rpw, min(256 * rpw, P), (nw - 1) * rpw, P})
    assert len(bounds) <= 16
    return bounds


def _pack_np(on):
    """bit g & 31 of word g >> 5, as int32 words."""
    P = on.size
    padded = np.zeros(((P + 31) // 32) * 32, dtype=np.uint8)
    padded[:P] = on
    return np.packbits(padded.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).view(np.int32)


# ---- pack --------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", SIZES)
def test_pack(P):
    rng = np.random.default_rng(P)
    count = rng.choice(np.array([0.0, 0.0, 1.0, 3.0, 1e-30], dtype=np.float32), size=P)
    if P > 4:
        count[:5] = [0.0, 1.0, 3.0, 1e-30, 0.0]
    words = torch.full(((P + 31) // 32,), -1, dtype=torch.int32, device=DEV)  # all ones
    out = _C().visibility_pack(torch.from_numpy(count).to(DEV), out=words)
    assert out is words
    np.testing.assert_array_equal(words.cpu().numpy(), _pack_np(count > 0))


def test_pack_allocates_and_checks():
    C = _C()
    w = C.visibility_pack(torch.ones(70, device=DEV))
    assert w.dtype == torch.int32 and w.shape == (3,)
    np.testing.assert_array_equal(w.cpu().numpy().view(np.uint32), [0xFFFFFFFF, 0xFFFFFFFF, 0x3F])
    with pytest.raises(RuntimeError, match="count"):
        C.visibility_pack(torch.ones(70, 1, device=DEV))
    with pytest.raises(RuntimeError, match="out"):
        C.visibility_pack(torch.ones(70, device=DEV), out=torch.zeros(2, dtype=torch.int32, device=DEV))
    assert C.visibility_pack(torch.ones(0, device=DEV)).numel() == 0


# ---- plan --------------------------------------------------------------------------------------
PATTERNS = ["none", "all", "first", "last", "half", "sparse", "disjoint", "identical"]


def _pattern(name, ranks, P, rng):
    on = np.zeros((ranks, P), dtype=bool)
    if name == "all":
        on[:] = True
    elif name == "first":
        on[0, 0] = True
    elif name == "last":
        on[ranks - 1, P - 1] = True
    elif name == "half":
        on = rng.random((ranks, P)) < 0.5 / ranks
    elif name == "sparse":
        on = rng.random((ranks, P)) < 0.02
    elif name == "disjoint":
        owner = rng.integers(0, ranks + 1, size=P)  # (owner == ranks: nobody)
        for r in range(ranks):
            on[r] = owner == r
    elif name == "identical":
        on[:] = rng.random(P) < 0.5
    return on


@pytest.mark.parametrize("ranks", [1, 2, 3])
def test_plan(ranks):
    C, rpw = _C(), _rpw()
    for P in _plan_sizes():
        bounds = _plan_bounds(P, rpw)
        for name in PATTERNS:
            rng = np.random.default_rng(1000 * ranks + P)
            on = _pattern(name, ranks, P, rng)
            words = torch.from_numpy(np.stack([_pack_np(r) for r in on])).to(DEV)
            rows = torch.full((P,), SENTINEL, dtype=torch.int32, device=DEV)
            mask = torch.ones((P,), dtype=torch.bool, device=DEV) if name == "none" else True
            U, rows_out, mask_out, below = C.union_plan(words, P, bounds=bounds, rows=rows, mask=mask)
            want = np.flatnonzero(on.any(axis=0))
            tag = f"ranks {ranks} P {P} {name}"
            assert U == want.size, tag
            got = rows_out.cpu().numpy()
            np.testing.assert_array_equal(got[:U], want, err_msg=tag)
            np.testing.assert_array_equal(got[U:], np.full(P - U, SENTINEL), err_msg=tag)
            np.testing.assert_array_equal(mask_out.cpu().numpy(), on.any(axis=0), err_msg=tag)
            assert below == [int((want < b).sum()) for b in bounds], tag


def test_plan_ignores_tail_bits_and_reuses_buffers():
    C = _C()
    P = 33
    words = torch.full((2, 2), -1, dtype=torch.int32, device=DEV)  # bits 33..63 set too
    ws = torch.empty((int(C.lib.gsr_union_workspace_size(P)),), dtype=torch.uint8, device=DEV)
    U, rows, mask, below = C.union_plan(words, P, bounds=[P], workspace=ws)
    assert U == P and below == [P] and mask is None
    np.testing.assert_array_equal(rows.cpu().numpy(), np.arange(P))
    U, _, _, below = C.union_plan(torch.zeros((1, 0), dtype=torch.int32, device=DEV), 0, bounds=[0])
    assert U == 0 and below == [0]


def test_plan_refusals():
    C, rpw = _C(), _rpw()
    P = 3 * rpw
    words = torch.zeros((1, P // 32), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="ranks"):
        C.union_plan(words[:0], P)
    with pytest.raises(RuntimeError, match="16"):
        C.union_plan(words, P, bounds=[0] * 17)
    with pytest.raises(RuntimeError, match="boundary"):
        C.union_plan(words, P, bounds=[rpw + 1])
    with pytest.raises(RuntimeError, match="boundary"):
        C.union_plan(words, P, bounds=[P + rpw])
    # the C entry point itself refuses what the binding catches first
    U = C._i(0)
    rc = C.lib.gsr_union_plan(P, 0, words.data_ptr(), 0, None, None, None, None, C.ctypes.byref(U), None, None)
    assert rc != 0 and b"ranks" in C.lib.gsr_last_error()
    rc = C.lib.gsr_union_plan(P, 1, words.data_ptr(), 17, (C._i * 17)(), None, None, None, C.ctypes.byref(U),
                              (C._i * 17)(), None)
    assert rc != 0 and b"n_bounds" in C.lib.gsr_last_error()


# ---- gather / scatter --------------------------------------------------------------------------
GROUP_SETS = [(3, 3, 45, 1, 3, 4, 1), (3, 3, 9, 1, 3, 4, 1), (3, 3, 24, 1, 3, 4, 1), (3, 3, 0, 1, 3, 4, 1)]


def _bits(shape, rng):
    """Random bit patterns viewed as float32 (NaNs and all): only an exact copy compares equal."""
    return torch.from_numpy(rng.integers(-2**31, 2**31 - 1, size=shape, dtype=np.int64).astype(np.int32)).to(DEV)


def _filled(n):
    return torch.full((n,), FILL, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("Ms", GROUP_SETS, ids=lambda m: f"rest{m[2]}")
def test_gather_scatter(Ms):
    C, mv = _C(), __import__("diff_gaussian_rasterization.multiview", fromlist=["x"])
    for P in (33, 1000, 2 * _rpw() + 5):
        rng = np.random.default_rng(P + sum(Ms))
        on = rng.random(P) < 0.5
        words = torch.from_numpy(_pack_np(on)[None]).to(DEV)
        U, rows, _, _ = C.union_plan(words, P)
        idx = torch.from_numpy(np.flatnonzero(on)).to(DEV)
        assert U == idx.numel() and U > 0
        src = [_bits((P, M), rng) for M in Ms]
        off = mv.compact_layout(U, Ms)
        assert off[-1] == U * sum(Ms)
        for u0, u1 in ((0, U), (0, U // 3), (U // 3, U), (U // 2, U // 2)):
            tag = f"P {P} window {(u0, u1)}"
            # gather: the window's elements of every group, nothing else (16 floats of slack behind)
            compact = _filled(off[-1] + 16)
            C.rows_gather([s.view(torch.float32) for s in src], rows, U, compact.view(torch.float32), window=(u0, u1))
            want = _filled(off[-1] + 16)
            for o, M, s in zip(off, Ms, src):
                want[o + u0 * M:o + u1 * M] = s.index_select(0, idx[u0:u1]).reshape(-1)
            assert torch.equal(compact, want), tag
            # scatter: the window's union rows of every group, no other row
            comp = _bits((off[-1],), rng)
            dst = [_filled(P * M).view(P, M) for M in Ms]
            C.rows_scatter([d.view(torch.float32) for d in dst], rows, U, comp.view(torch.float32), window=(u0, u1))
            for o, M, d in zip(off, Ms, dst):
                w = _filled(P * M).view(P, M)
                w[idx[u0:u1]] = comp[o + u0 * M:o + u1 * M].view(u1 - u0, M)
                assert torch.equal(d, w), tag


def test_gather_then_scatter_through_a_large_plan():
    """256 waves and one row (union_offsets_kernel's threads own two waves each), a `half` union of
    about 130k rows: rows_gather then rows_scatter through the plan's own `rows`, over a window that
    starts and ends off a workgroup's 256 elements, bitwise against index_select / index_copy_ with
    numpy's flatnonzero."""
    C, mv = _C(), __import__("diff_gaussian_rasterization.multiview", fromlist=["x"])
    P, Ms = 256 * _rpw() + 1, (3, 45, 1)
    rng = np.random.default_rng(P)
    on = _pattern("half", 1, P, rng)[0]
    U, rows, _, _ = C.union_plan(torch.from_numpy(_pack_np(on)[None]).to(DEV), P)
    idx = torch.from_numpy(np.flatnonzero(on)).to(DEV)
    assert U == idx.numel() and 120_000 < U < 140_000
    assert torch.equal(rows[:U].long(), idx)
    u0, u1 = 100 * 256 + 37, U - 91
    assert u0 % 256 and u1 % 256 and all(((u1 - u0) * M) % 256 and (u0 * M) % 256 for M in Ms)
    src = [_bits((P, M), rng) for M in Ms]
    off = mv.compact_layout(U, Ms)
    compact = _filled(off[-1] + 16)
    C.rows_gather([s.view(torch.float32) for s in src], rows, U, compact.view(torch.float32), window=(u0, u1))
    want = _filled(off[-1] + 16)
    for o, M, s in zip(off, Ms, src):
        want[o + u0 * M:o + u1 * M] = s.index_select(0, idx[u0:u1]).reshape(-1)
    assert torch.equal(compact, want)
    dst = [_filled(P * M).view(P, M) for M in Ms]
    C.rows_scatter([d.view(torch.float32) for d in dst], rows, U, compact.view(torch.float32), window=(u0, u1))
    for M, s, d in zip(Ms, src, dst):
        w = _filled(P * M).view(P, M)
        w.index_copy_(0, idx[u0:u1], s.index_select(0, idx[u0:u1]))
        assert torch.equal(d, w), M


def test_gather_then_scatter_round_trip_leaves_other_rows():
    C = _C()
    P, Ms = 1000, (3, 3, 45, 1, 3, 4, 1)
    rng = np.random.default_rng(7)
    on = rng.random(P) < 0.5
    U, rows, mask, _ = C.union_plan(torch.from_numpy(_pack_np(on)[None]).to(DEV), P, mask=True)
    src = [_bits((P, M), rng) for M in Ms]
    keep = [s.clone() for s in src]
    compact = torch.empty(U * sum(Ms), device=DEV)
    C.rows_gather([s.view(torch.float32) for s in src], rows, U, compact)
    for s in src:
        s[mask] = 0
    C.rows_scatter([s.view(torch.float32) for s in src], rows, U, compact)
    for s, k in zip(src, keep):
        assert torch.equal(s, k)


def test_move_refusals():
    C = _C()
    P, U = 64, 10
    t = [torch.zeros(P, 3, device=DEV)]
    rows = torch.arange(P, dtype=torch.int32, device=DEV)
    compact = torch.zeros(P * 3, device=DEV)
    for fn in (C.rows_gather, C.rows_scatter):
        for window in ((-1, 5), (0, U + 1), (6, 5)):
            with pytest.raises(RuntimeError, match="window"):
                fn(t, rows, U, compact, window=window)
        with pytest.raises(RuntimeError, match="8 groups"):
            fn(t * 9, rows, U, torch.zeros(P * 27, device=DEV))
        fn(t, rows, 0, compact)  # U == 0: nothing to do
    n = 9
    rc = C.lib.gsr_rows_gather(P, U, 0, U, n, (C._i * n)(*[3] * n), (C._vp * n)(*[t[0].data_ptr()] * n),
                               rows.data_ptr(), compact.data_ptr(), None)
    assert rc != 0 and b"n_groups" in C.lib.gsr_last_error()
    rc = C.lib.gsr_rows_scatter(P, P + 1, 0, 1, 1, (C._i * 1)(3), (C._vp * 1)(t[0].data_ptr()), rows.data_ptr(),
                                compact.data_ptr(), None)
    assert rc != 0 and b"U must be" in C.lib.gsr_last_error()
    # U * M >= 2^32 - 16 is refused before anything is launched (no memory of that size is touched)
    big_P = 2**31 - 1
    rc = C.lib.gsr_rows_gather(big_P, big_P, 0, 1, 1, (C._i * 1)(3), (C._vp * 1)(t[0].data_ptr()), rows.data_ptr(),
                               compact.data_ptr(), None)
    assert rc != 0 and b"2^32" in C.lib.gsr_last_error()
