"""Every launch branch of the batched GMRES on the device (pf_krylov_solve, csrc/krylov.hip) against exact fp64 solutions.
Needs a real MI355X:  python -m pytest tests/test_gpu_krylov_paths.py -m gpu -s

The case table, the right-hand sides and the exact solutions are tests/krylov_reference.py (pinned on the CPU by tests/test_krylov_reference_host.py);
tests/golden/krylov_paths.npz holds what the REAL reference's utils.GMRES does on the same systems in fp32 (tools/make_golden_spatial.py gmres_paths):
its Krylov vector counts and, per image, d_ref = max|ref32 - exact| (capped cases: - gmres64's iterate at the cap).

Parity, per image:  converged cases  max|hip - exact| <= max(4 d_ref, (k + 2) 2^-23 max|exact|)  - 4 x the reference's own distance (the margin of
DESIGN.md 4.20), with the rounding of the k fp32 FMAs of krylov_combine_kernel plus the normalisation and the fp32 cast of y as a floor (d_ref = 0
would otherwise ask for bit equality with a differently ordered algorithm); capped cases  max|hip - gmres64 iterate| <= 4 d_ref.  Counts: within 1
of the reference's where the tool asserted that the fp32 and fp64 references agree within 1, exactly max_iter on the capped cases, 0 and a bit-equal
copy where the right-hand side is returned.  Everything else here is bit for bit.

Measured on the MI355X, largest over the images (d_ref beside it):  zs 7.02e-5 (1.681e-4), zv 7.70e-5 (2.046e-4), z3k43 3.21e-5 and z3k61 3.49e-5
(1.329e-4), pc 7.54e-5 (6.606e-5), pc128 9.96e-5 (6.791e-5), gc 9.44e-5 (1.052e-4), pz 3.42e-5 (4.069e-5), dn 1.93e-6 (3.491e-6), bx 1.51e-5
(3.830e-5), mk 4.21e-5 (4.213e-5), cap5 2.01e-5 (4.191e-5), zvcap5 2.01e-5 (6.276e-5), dzcap5 1.76e-5 (5.005e-5), cap256 3.14e-1 (6.535e-1,
max|sol| 6.07e3), mix 5.87e-5 (1.016e-4).  The counts equal the reference's everywhere but on pc128 (33; reference 35, fp64 33) and gc (34, 14;
reference 36, 14, fp64 34, 14), two of the cases on which none is compared.
The table with shapes and counts: DESIGN.md 4.20.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import krylov_reference as K

pytestmark = pytest.mark.gpu

GUARD = 4096
PF_ERR_INVALID = -1


@pytest.fixture(scope="module")
def hip():
    import pnpflow_amd._lib as L
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    L.load()
    return L


def sentinel(dtype):
    """a finite pattern no kernel would write by accident"""
    return (torch.arange(GUARD, device="cuda") * 3 + 12345).to(dtype)


def bits(t):
    return t.view(torch.int32)


def descriptor(L, name, images=None):
    """the case's pf_degradation and the device tensors it points to (kept alive by the caller)"""
    c = K.CASES[name]
    d = L.PfDegradation(); d.kind = c["kind"]; d.half_size_mask = int(c["half"])
    keep = []
    taps = K.taps_of(c)
    if taps is not None:
        t = torch.from_numpy(np.ascontiguousarray(taps, dtype=np.float32)).cuda()
        d.ntaps = int(taps.shape[0]); d.taps = t.data_ptr(); keep.append(t)
    if c["kind"] == 2:
        m = K.mask_of(c)
        m = torch.from_numpy(np.ascontiguousarray(m if images is None else m[images])).cuda()
        d.mask = m.data_ptr(); keep.append(m)
    return d, keep


def solve(L, name, images=None, max_iter=None, rhs=None, offset=0, guard=False, kind=None, ws_floats_delta=0, ws_offset=0, alias=False, replay=None):
    """One pf_krylov_solve of case `name` (or of its images `images`) -> (rc, sol, iters) as numpy.  NaN-filled workspace of exactly
    pf_krylov_workspace_floats floats, NaN-filled sol, iters = -7.  offset: rhs and sol are views `offset` floats into larger buffers.
    guard: GUARD sentinel elements behind the workspace, sol and iters, asserted untouched.  replay: a callable that gets (call, reset) and drives
    the call itself (stream capture)."""
    lib = L.load()
    c = K.CASES[name]
    r = np.array(K.rhs(name) if rhs is None else rhs)
    rt2 = K.rt2_of(name)
    if images is not None:
        r, rt2 = r[images], rt2[images]
    B, Cc, H, W = r.shape
    N = r.size
    mi = c["max_iter"] if max_iter is None else max_iter
    d, keep = descriptor(L, name, images)
    if kind is not None:
        d.kind = kind; d.sf = 2
    nws = int(lib.pf_krylov_workspace_floats(B, Cc, H, W, max(min(mi, K.KR_MAXM), 0)))
    assert nws >= (max(mi, 1) + 3) * N or mi > K.KR_MAXM
    extra = GUARD if guard else 0
    ws = torch.full((nws + ws_offset + extra,), float("nan"), device="cuda")
    rbuf = torch.zeros((N + offset + 4,), device="cuda")
    sbuf = torch.full((N + offset + extra,), float("nan"), device="cuda")
    ibuf = torch.full((B + extra,), -7, dtype=torch.int32, device="cuda")
    rbuf[offset:offset + N] = torch.from_numpy(r.reshape(-1)).cuda()
    if guard:
        ws[nws:] = sentinel(torch.float32); sbuf[offset + N:] = sentinel(torch.float32); ibuf[B:] = sentinel(torch.int32)
    rt2_d = torch.from_numpy(rt2).cuda()
    sol_ptr = sbuf.data_ptr() + 4 * offset
    rhs_ptr = sol_ptr if alias else rbuf.data_ptr() + 4 * offset
    assert ws.data_ptr() % 16 == 0 and rbuf.data_ptr() % 16 == 0 and sbuf.data_ptr() % 16 == 0
    torch.cuda.synchronize()

    def call():
        return lib.pf_krylov_solve(C.byref(d), rt2_d.data_ptr(), float(np.float32(c["sigma2"])), rhs_ptr, sol_ptr, B, Cc, H, W, mi, K.TOL, K.ATOL,
                                   ws.data_ptr() + 4 * ws_offset, nws + ws_floats_delta, ibuf.data_ptr(), L.current_stream_ptr())

    def reset():
        ws[:nws + ws_offset] = float("nan"); sbuf[:offset + N] = float("nan"); ibuf[:B] = -7
        torch.cuda.synchronize()

    def result():
        torch.cuda.synchronize()
        if guard:
            assert torch.equal(bits(ws[nws:]), bits(sentinel(torch.float32))), "the solve wrote behind its workspace"
            assert torch.equal(bits(sbuf[offset + N:]), bits(sentinel(torch.float32))), "the solve wrote behind sol"
            assert torch.equal(ibuf[B:], sentinel(torch.int32)), "the solve wrote behind iters"
        assert torch.isnan(sbuf[:offset]).all()
        return sbuf[offset:offset + N].reshape(r.shape).cpu().numpy(), ibuf[:B].cpu().numpy()

    if replay is not None:
        return replay(call, reset, result)
    rc = call()
    return (rc,) + result()


_RUNS = {}


def full_run(L, name):
    """the plain solve of a table case, run once and shared (read-only)"""
    if name not in _RUNS:
        rc, sol, iters = solve(L, name)
        assert rc == 0, (name, rc)
        sol.setflags(write=False); iters.setflags(write=False)
        _RUNS[name] = (sol, iters)
    return _RUNS[name]


def same(a, b):
    """bit for bit, NaN payloads included"""
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# parity
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.CASES))
def test_solve_matches_the_exact_solution(hip, golden, name):
    c, g = K.CASES[name], golden("krylov_paths")
    i32, dref, solmax = g[f"{name}_iters32"], g[f"{name}_dref"], g[f"{name}_solmax"]
    if c["kind"] in (4, 6):         # the table's taps are the Python operator's
        import pnpflow_amd.degradations as D
        deg = D.GaussianDeblurring(c["blur"], 61, "fft" if c["kind"] == 4 else "spatial")
        assert deg.kind == c["kind"] and np.array_equal(K.taps_of(c), deg.taps_eff if c["visible"] else deg.taps_host)
    sol, iters = full_run(hip, name)
    target = K.gmres64(name)[0] if c["capped"] else K.exact(name)
    ret = K.returns_rhs(name)
    B = c["shape"][0]
    err = np.abs(sol.astype(np.float64) - target).reshape(B, -1).max(axis=1)
    tol = 4 * dref if c["capped"] else np.maximum(4 * dref, (i32 + 2) * 2.0 ** -23 * solmax)
    print(f"krylov {name}: max|hip - {'gmres64' if c['capped'] else 'exact'}| = {['%.3e' % e for e in err]} (tolerance {['%.3e' % t for t in tol]}, "
          f"d_ref {['%.3e' % v for v in dref]}), Krylov vectors {iters.tolist()} (reference {i32.tolist()}, fp64 {g[f'{name}_iters64'].tolist()})")
    assert np.isfinite(sol).all()
    for b in range(B):
        if ret[b]:
            assert iters[b] == 0 and same(sol[b], K.rhs(name)[b]), f"image {b}: the right-hand side is returned"
        else:
            assert iters[b] > 0 and err[b] <= tol[b], f"image {b}: {err[b]:.3e} > {tol[b]:.3e}"
    if c["capped"]:
        assert (iters == c["max_iter"]).all(), iters
    elif c["counts"]:
        assert np.abs(iters - i32).max() <= 1, (iters, i32)
    # (a) two runs agree bit for bit
    rc, sol2, iters2 = solve(hip, name)
    assert rc == 0 and same(sol, sol2) and np.array_equal(iters, iters2)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# invariants without a tolerance
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zs", "pc", "mix"])
def test_image_of_a_batch_equals_its_own_solve(hip, name):
    """(b) masked iterations never touch a finished image, and no reduction crosses images"""
    sol, iters = full_run(hip, name)
    for b in range(K.CASES[name]["shape"][0]):
        rc, s1, i1 = solve(hip, name, images=[b])
        assert rc == 0 and i1[0] == iters[b] and same(s1[0], sol[b]), (name, b, i1, iters)


@pytest.mark.parametrize("name", ["z3k43", "z3k61", "pc"])
def test_misaligned_views_equal_the_aligned_run(hip, name):
    """(c) rhs and sol one float into larger buffers: n % 4 == 0 with misaligned pointers takes the scalar instantiations, which walk the same quads
    in the same order"""
    assert K.n_of(K.CASES[name]) % 4 == 0
    sol, iters = full_run(hip, name)
    rc, s1, i1 = solve(hip, name, offset=1, guard=True)
    assert rc == 0 and np.array_equal(i1, iters) and same(s1, sol)


def test_max_iter_zero_returns_the_right_hand_side(hip):
    """(d)"""
    rc, sol, iters = solve(hip, "zs", max_iter=0, guard=True)
    assert rc == 0 and (iters == 0).all() and same(sol, np.array(K.rhs("zs")))


def test_nan_right_hand_side_stops_its_image_alone(hip):
    """(e) the documented !(res == res) exit: NaN arithmetic, not a fault"""
    sol, iters = full_run(hip, "mix")
    r = np.array(K.rhs("mix"))
    r[0] = np.nan
    rc, s1, i1 = solve(hip, "mix", rhs=r)
    assert rc == 0
    assert np.array_equal(i1[1:], iters[1:]) and same(s1[1:], sol[1:])
    assert i1[0] == 1 and not np.isfinite(s1[0]).any()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# workspace contract
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zs", "cap256"])
def test_nothing_is_written_behind_the_buffers(hip, name):
    sol, iters = full_run(hip, name)
    rc, s1, i1 = solve(hip, name, guard=True)           # (solve() asserts the sentinels)
    assert rc == 0 and same(s1, sol) and np.array_equal(i1, iters)


REFUSALS = {
    "workspace one float short": dict(ws_floats_delta=-1),
    "workspace off alignment": dict(ws_offset=1),
    "max_iter 257": dict(max_iter=257),
    "max_iter -1": dict(max_iter=-1),
    "rhs == sol": dict(alias=True),
    "kind 3": dict(kind=3),
    "kind 5": dict(kind=5),
    "kind 9": dict(kind=9),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals_leave_sol_untouched(hip, what):
    # kinds 3 and 5 on z3's separable descriptor, kind 9 on pc's 21 x 21 kernel (sf = 2 divides both shapes): only the kind itself is at fault
    rc, sol, iters = solve(hip, "pc" if what == "kind 9" else "z3k43", **REFUSALS[what])
    assert rc == PF_ERR_INVALID, (what, rc)
    assert np.isnan(sol).all() and (iters == -7).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# stream capture
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_captured_solve_replays_bit_for_bit(hip):
    """the documented no-poll loop: under capture the host never reads the flags and enqueues max_iter masked iterations"""
    rc, sol, iters = solve(hip, "zs", max_iter=12)
    assert rc == 0 and (iters == 12).all(), (rc, iters)       # (the reference needs at least 14 vectors on every image of zs)

    def replay(call, reset, result):
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            assert call() == 0                          # once outside capture on this stream: every kernel is loaded
        side.synchronize()
        reset()
        with torch.cuda.graph(graph, stream=side):
            rcc = call()
        assert rcc == 0
        out = []
        for _ in range(3):
            reset()
            graph.replay()
            out.append(result())
        return out

    for s1, i1 in solve(hip, "zs", max_iter=12, replay=replay):
        assert same(s1, sol) and np.array_equal(i1, iters)
