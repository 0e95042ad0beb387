"""Every BatchNorm entry point of csrc/bn.hip against the plain fp64 reference tests/bn_ref.py:
the slice kernels (fh_bn_fwd_train / _stats / _eval, fh_bn_bwd, fh_bn_bwd_pool) and the tile
kernels (fh_bn_finalize_tiles, fh_bn_apply_tiles, fh_maxpool2_fwd_bnfinalize, fh_bn_bwd_tiles,
fh_bn_bwd_pool_tiles), whose per-tile fp64 statistics are built on the host from the reference.

Shapes and counts: tests/bn_cases.py (odd channel counts, scalar and float4 paths, 63 / 64 / 65
tiles, slice edges, clients with the full batch, a ragged count, one image and none).  Layout:
gamma / beta / dgamma / dbeta are column views of wider rows at a non-zero offset (row stride
!= C), the running statistics and scale / shift likewise; every output is pre-filled with a
sentinel, every input image past a client's count holds NaN.

Tolerances are those of tests/test_layers_gpu.py, applied per channel.  The mean-100 channel's
y, dx and dgamma are bounded by four times the error of F.batch_norm in float32 on the CPU
against the same fp64 reference (see _ill_bound)."""
import pytest
import torch

import bn_cases
import bn_ref
from bn_cases import ILL, case_id
from fedhip import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENT = bn_ref.SENTINEL
NAN = float("nan")


# ------------------------------------------------------------------ helpers
def _ulps(a, b):
    """Largest distance in units in the last place between two fp32 tensors."""
    ia = a.contiguous().view(torch.int32).to(torch.int64)
    ib = b.contiguous().view(torch.int32).to(torch.int64)
    ia = torch.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = torch.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int((ia - ib).abs().max())


def _poison(t, counts, value=NAN):
    """Copy of t [clients, batch, ...] with every image past a client's count overwritten."""
    t = t.clone()
    for z, n in enumerate(counts):
        t[z, n:] = value
    return t


class Rows:
    """[clients, width] sentinel-filled rows; take() hands out [clients, C] column views at
    growing non-zero offsets, so the row stride differs from C."""

    def __init__(self, nc, C, slots):
        self.C = C
        self.buf = torch.full((nc, 3 + slots * (C + 2)), SENT, device=DEV)
        self.used = []

    def take(self, init=None):
        o = 3 + len(self.used) * (self.C + 2)
        v = self.buf[:, o:o + self.C]
        if init is not None:
            v.copy_(init)
        self.used.append(o)
        assert v.stride(0) != self.C and v.data_ptr() != self.buf.data_ptr()
        return v

    def gaps_intact(self):
        keep = torch.ones(self.buf.shape[1], dtype=torch.bool)
        for o in self.used:
            keep[o:o + self.C] = False
        return bool((self.buf[:, keep.to(DEV)] == SENT).all())


class Dev:
    """Device copies of a case's inputs, laid out as described in the module docstring."""

    def __init__(self, c):
        nc, B, C, H, W = c.shape
        self.c = c
        self.counts = torch.tensor(c.counts, dtype=torch.int32, device=DEV)
        self.x = _poison(c.x, c.counts).to(DEV)
        self.params = Rows(nc, C, 2)
        self.gamma, self.beta = self.params.take(c.gamma), self.params.take(c.beta)

    def running(self):
        r = Rows(self.c.shape[0], self.c.shape[2], 2)
        return r, r.take(self.c.rmean0), r.take(self.c.rvar0)

    def pair(self):
        r = Rows(self.c.shape[0], self.c.shape[2], 2)
        return r, r.take(), r.take()

    def saved(self):
        nc, C = self.c.shape[0], self.c.shape[2]
        return torch.full((nc, C), SENT, device=DEV), torch.full((nc, C), SENT, device=DEV)

    def saved_ref(self):
        """save_mean / save_invstd as the forward leaves them: the fp64 values rounded."""
        sm = torch.stack([s.mean for s in self.c.stats]).float()
        si = torch.stack([s.invstd for s in self.c.stats]).float()
        return sm, si

    def fwd_part(self):
        return torch.stack([bn_ref.fwd_tiles(self.c.x[z], n)
                            for z, n in enumerate(self.c.counts)]).to(DEV)


def _check_stats(d, sm, si, rrows, rm, rv, srows=None, sc=None, sh=None):
    """save_mean / save_invstd within 1 ulp of the rounded fp64 value; running statistics and
    scale / shift within rtol 1e-5 / atol 1e-6; a client with no image: 0, 0 and the running
    statistics bit-unchanged; no NaN; nothing written between the column views."""
    c = d.c
    torch.cuda.synchronize()
    for t in (sm, si, rm, rv) + ((sc, sh) if sc is not None else ()):
        assert not torch.isnan(t).any()
    for z, n in enumerate(c.counts):
        st = c.stats[z]
        assert _ulps(sm[z].cpu(), st.mean.float()) <= 1, (z, sm[z], st.mean)
        assert _ulps(si[z].cpu(), st.invstd.float()) <= 1, (z, si[z], st.invstd)
        if n == 0:
            assert bool((sm[z] == 0).all()) and bool((si[z] == 0).all())
            assert torch.equal(rm[z].cpu(), c.rmean0[z]) and torch.equal(rv[z].cpu(), c.rvar0[z])
        tol = dict(rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(rm[z].double().cpu(), st.rmean, **tol)
        torch.testing.assert_close(rv[z].double().cpu(), st.rvar, **tol)
        if sc is not None:
            torch.testing.assert_close(sc[z].double().cpu(), st.scale, **tol)
            torch.testing.assert_close(sh[z].double().cpu(), st.shift, **tol)
    assert rrows.gaps_intact() and d.params.gaps_intact()
    assert srows is None or srows.gaps_intact()


def _ill_bound(what, err, err32):
    """The mean-100 channel: the kernel's largest error against fp64 may be four times that
    of the same computation in float32 on the CPU (another summation order, the same
    formulation).  Prints both figures (pytest -s / -rP shows them)."""
    print(f"ill-conditioned channel {what}: kernel {err:.3e}  cpu-fp32 {err32:.3e}")
    assert err <= 4.0 * err32, (what, err, err32)


def _check_rows_past_count(t, counts, fill=SENT):
    for z, n in enumerate(counts):
        assert bool((t[z, n:] == fill).all()), z


def _check_y(c, y, refs, rel):
    """y [clients, batch, C, h, w] against the per-client fp64 refs (None for n == 0): every
    channel but the mean-100 one within rel * (1 + max|ref|) of that channel; the sentinel
    past the count."""
    y = y.cpu()
    _check_rows_past_count(y, c.counts)
    for z, n in enumerate(c.counts):
        if n == 0:
            continue
        ref = refs[z]
        assert not torch.isnan(y[z, :n]).any()
        err = (y[z, :n].double() - ref).abs().amax((0, 2, 3))
        lim = rel * (1 + ref.abs().amax((0, 2, 3)))
        ok = err <= lim
        ok[ILL] = True
        assert bool(ok.all()), (z, err, lim)


def _check_y_ill(c, y, refs, units32, what, gain=1.0):
    """The mean-100 channel of y by _ill_bound, every client on its own.  Both figures are in
    ulps of the client's shift (bn_cases.ill_unit); units32 is the float32 CPU figure over
    all cases, because a single client's error is one draw of two roundings, not a
    measurement (see bn_cases.cpu_fp32_y_units)."""
    y = y.cpu()
    for z, n in enumerate(c.counts):
        if n:
            _ill_bound(f"{what} client {z}", bn_cases.ill_units(c, z, y[z, :n], refs[z], gain),
                       units32)


# ------------------------------------------------------------------ forward statistics
@pytest.mark.parametrize("case", bn_cases.CASES, ids=case_id)
@pytest.mark.parametrize("kind", ["fwd_stats", "finalize_tiles"])
def test_stats(case, kind):
    c = bn_cases.build(*case)
    nc, B, C, H, W = c.shape
    d = Dev(c)
    rrows, rm, rv = d.running()
    srows, sc, sh = d.pair()
    sm, si = d.saved()
    if kind == "fwd_stats":
        ops.bn_fwd_stats(d.x, d.gamma, d.beta, rm, rv, sm, si, sc, sh, nc, B, C, H * W,
                         counts=d.counts)
    else:
        ops.bn_finalize_tiles(d.fwd_part(), d.gamma, d.beta, rm, rv, sm, si, sc, sh, nc, B, C,
                              H * W, counts=d.counts)
    _check_stats(d, sm, si, rrows, rm, rv, srows, sc, sh)


VARIANTS = ((False, False), (True, False), (True, True), (False, True))  # (relu, residual)


def _run_apply(d, kind, part, res_dev, relu, residual):
    c = d.c
    nc, B, C, H, W = c.shape
    rrows, rm, rv = d.running()
    sm, si = d.saved()
    y = torch.full_like(d.x, SENT)
    r = res_dev if residual else None
    if kind == "fwd_train":
        ops.bn_fwd_train(d.x, y, d.gamma, d.beta, rm, rv, sm, si, nc, B, C, H * W, relu=relu,
                         res=r, counts=d.counts)
    else:
        ops.bn_apply_tiles(part, d.x, y, d.gamma, d.beta, rm, rv, sm, si, nc, B, C, H * W,
                           relu=relu, res=r, counts=d.counts)
    refs = [c.y_ref(z, relu, residual) if n else None for z, n in enumerate(c.counts)]
    return y, refs, (sm, si, rrows, rm, rv)


@pytest.mark.parametrize("case", bn_cases.CASES, ids=case_id)
@pytest.mark.parametrize("kind", ["fwd_train", "apply_tiles"])
def test_apply(case, kind):
    c = bn_cases.build(*case)
    d = Dev(c)
    res_dev = _poison(c.res, c.counts).to(DEV)
    part = d.fwd_part() if kind == "apply_tiles" else None
    for relu, residual in VARIANTS:
        y, refs, stats = _run_apply(d, kind, part, res_dev, relu, residual)
        _check_stats(d, *stats)
        _check_y(c, y, refs, 2e-5)


@pytest.mark.parametrize("case", bn_cases.CASES, ids=case_id)
@pytest.mark.parametrize("kind", ["fwd_train", "apply_tiles"])
def test_apply_ill_conditioned_channel(case, kind):
    """y on the mean-100, std-0.01 channel: every client's largest error at most four times
    the largest error of F.batch_norm in float32 on the CPU, both against fp64 and in ulps of
    the client's shift (2^-23 |beta - mean*scale|, about 1e-3 here)."""
    c = bn_cases.build(*case)
    d = Dev(c)
    res_dev = _poison(c.res, c.counts).to(DEV)
    part = d.fwd_part() if kind == "apply_tiles" else None
    for relu, residual in VARIANTS:
        y, refs, _ = _run_apply(d, kind, part, res_dev, relu, residual)
        # measured: cpu-fp32 0.622 ulp of the shift (largest of 48 clients, each of the four
        # variants) -> bound 2.49 ulp; kernel on an MI355X 1.317 ulp (1x2x5x2x2-n1, both
        # entry points; median 0.54).  The kernels build without FMA contraction: fl(mean),
        # fl(mean*alpha), fl(beta - .) and fl(x*alpha) are four roundings of at most half an
        # ulp of the shift each, 2.0 ulp in the worst case, so the bound holds for any input
        _check_y_ill(c, y, refs, bn_cases.cpu_fp32_y_units(relu, residual),
                     f"y relu={relu} res={residual}")


def _run_pool_finalize(d, drop_mode):
    c = d.c
    nc, B, C, H, W = c.shape
    p = 0.5 if drop_mode else 0.0
    rrows, rm, rv = d.running()
    srows, sc, sh = d.pair()
    sm, si = d.saved()
    q = torch.full((nc, B, C, H // 2, W // 2), SENT, device=DEV)
    idx = torch.full(q.shape, 255, dtype=torch.uint8, device=DEV)
    mask = c.pmask.to(DEV) if drop_mode else None
    ops.maxpool2_fwd_bnfinalize(d.fwd_part(), d.gamma, d.beta, rm, rv, sm, si, sc, sh, d.x, q,
                                idx, nc, B, C, H, W, mask=mask, drop_mode=drop_mode, p_drop=p,
                                counts=d.counts)
    refs = [c.pool_ref(z, c.pmask if drop_mode else None, p) if n else None
            for z, n in enumerate(c.counts)]
    return q, idx, mask, refs, (sm, si, rrows, rm, rv, srows, sc, sh)


@pytest.mark.parametrize("case", bn_cases.POOL_CASES, ids=case_id)
@pytest.mark.parametrize("drop_mode", [0, 2])
def test_pool_finalize(case, drop_mode):
    c = bn_cases.build(*case)
    d = Dev(c)
    q, idx, mask, refs, stats = _run_pool_finalize(d, drop_mode)
    _check_stats(d, *stats)
    if drop_mode:
        assert torch.equal(mask.cpu(), c.pmask)   # mode 2 reads the mask, never writes it
    idx = idx.cpu()
    _check_rows_past_count(idx, c.counts, 255)
    for z, n in enumerate(c.counts):
        if n:
            _, ir, near = refs[z]
            assert torch.equal(idx[z, :n][~near], ir[~near]), z
    _check_y(c, q, [r[0] if r else None for r in refs], 2e-5)


@pytest.mark.parametrize("case", bn_cases.POOL_CASES, ids=case_id)
@pytest.mark.parametrize("drop_mode", [0, 2])
def test_pool_finalize_ill_conditioned_channel(case, drop_mode):
    """The pooled y on the mean-100 channel, bounded like test_apply_ill_conditioned_channel;
    a kept element's factor 1/(1-p) = 2 is exact and divided out of both figures."""
    c = bn_cases.build(*case)
    d = Dev(c)
    q, _, _, refs, _ = _run_pool_finalize(d, drop_mode)
    # measured: cpu-fp32 0.589 ulp of the shift (largest of 37 clients, either drop mode)
    # -> bound 2.35 ulp; kernel on an MI355X 1.164 ulp (1x2x5x2x2-n1; median 0.54)
    _check_y_ill(c, q, [r[0] if r else None for r in refs],
                 bn_cases.cpu_fp32_pool_units(bool(drop_mode)),
                 f"pooled y drop_mode={drop_mode}", gain=2.0 if drop_mode else 1.0)


# ------------------------------------------------------------------ eval
@pytest.mark.parametrize("case", bn_cases.EVAL_CASES, ids=case_id)
def test_eval(case):
    c = bn_cases.build(*case)
    nc, B, C, H, W = c.shape
    d = Dev(c)
    res_dev = _poison(c.res, c.counts).to(DEV)
    for relu, residual in ((False, False), (False, True), (True, True), (True, False)):
        rrows, rm, rv = d.running()
        y = torch.full_like(d.x, SENT)
        ops.bn_fwd_eval(d.x, y, d.gamma, d.beta, rm, rv, nc, B, C, H * W, relu=relu,
                        res=res_dev if residual else None, counts=d.counts)
        torch.cuda.synchronize()
        y = y.cpu()
        _check_rows_past_count(y, c.counts)
        assert torch.equal(rm.cpu(), c.rmean0) and torch.equal(rv.cpu(), c.rvar0)
        assert rrows.gaps_intact()
        for z, n in enumerate(c.counts):
            if n == 0:
                continue
            inv = 1.0 / torch.sqrt(c.rvar0[z].double() + bn_ref.EPS)
            scale = inv * c.gamma[z].double()
            shift = c.beta[z].double() - c.rmean0[z].double() * scale
            ref = bn_ref.apply(c.x[z, :n], scale, shift, c.res[z, :n] if residual else None, relu)
            err = (y[z, :n].double() - ref).abs().max().item()
            assert err <= 1e-5 * (1 + ref.abs().max().item()), (z, err)


# ------------------------------------------------------------------ backward
def _check_bwd(c, dx, dg, db, grows, gs, what):
    """dx per channel within 1e-4 * max|ref dx| + 1e-6, dgamma / dbeta within rtol 1e-4 /
    atol 1e-4 of the fp64 reference for the gradients gs (per client, ReLU mask applied);
    the mean-100 channel's dx and dgamma by _ill_bound; sentinel past the count; a client
    with no image: dgamma == dbeta == 0 and dx untouched."""
    torch.cuda.synchronize()
    dx, dg, db = dx.cpu(), dg.cpu(), db.cpu()
    _check_rows_past_count(dx, c.counts)
    assert grows.gaps_intact()
    assert not torch.isnan(dg).any() and not torch.isnan(db).any()
    ill = ill32 = illg = illg32 = 0.0
    for z, n in enumerate(c.counts):
        st = c.stats[z]
        rdx, rdg, rdb = bn_ref.bwd(gs[z], c.x[z], st.mean, st.invstd, c.gamma[z], n)
        if n == 0:
            assert bool((dg[z] == 0).all()) and bool((db[z] == 0).all())
            continue
        assert not torch.isnan(dx[z, :n]).any()
        err = (dx[z, :n].double() - rdx).abs().amax((0, 2, 3))
        lim = 1e-4 * rdx.abs().amax((0, 2, 3)) + 1e-6
        ok = err <= lim
        ok[ILL] = True
        assert bool(ok.all()), (z, err, lim)
        gerr = (dg[z].double() - rdg).abs()
        gok = gerr <= 1e-4 + 1e-4 * rdg.abs()
        gok[ILL] = True
        assert bool(gok.all()), (z, gerr, rdg)
        torch.testing.assert_close(db[z].double(), rdb, rtol=1e-4, atol=1e-4)
        dx32, dg32 = c.bwd_f32(z, gs[z][:n])
        ill = max(ill, err[ILL].item())
        ill32 = max(ill32, (dx32[:, ILL].double() - rdx[:, ILL]).abs().max().item())
        illg = max(illg, gerr[ILL].item())
        illg32 = max(illg32, abs(dg32[ILL].item() - rdg[ILL].item()))
    # measured on an MI355X, largest over all cases and entry points: dx kernel 1.488e-01,
    # cpu-fp32 1.487e-01 (largest kernel / cpu ratio of any case 1.012); dgamma kernel
    # 4.647e-02, cpu-fp32 4.650e-02 (largest ratio 1.037): both use fl(mean)
    _ill_bound("dx " + what, ill, ill32)
    # dgamma of this channel inherits fl(mean)'s error times invstd * sum g: the inherited
    # tolerance where it suffices, else the float32 CPU figure
    if illg > 1e-4:
        _ill_bound("dgamma " + what, illg, illg32)


def _bwd_outputs(d):
    grows, dg, db = d.pair()
    return torch.full_like(d.x, SENT), grows, dg, db


@pytest.mark.parametrize("case", bn_cases.CASES, ids=case_id)
def test_bwd(case):
    """fh_bn_bwd: no ReLU; ReLU with the stored output; ReLU recomputed from x and beta; ReLU
    after a residual add (stored output, dres exact)."""
    c = bn_cases.build(*case)
    nc, B, C, H, W = c.shape
    d = Dev(c)
    sm, si = (t.to(DEV) for t in d.saved_ref())
    dy_dev = _poison(c.dy, c.counts).to(DEV)
    for relu, residual, recompute in ((False, False, False), (True, False, False),
                                      (True, False, True), (True, True, False),
                                      (False, True, False)):
        yref = [c.y_ref(z, relu, residual) for z in range(nc)]
        gs = [c.dy[z, :n] * (yref[z] > 0) if relu else c.dy[z, :n]
              for z, n in enumerate(c.counts)]
        yout = None
        if relu and not recompute:
            yout = torch.full(c.x.shape, NAN)
            for z, n in enumerate(c.counts):
                yout[z, :n] = yref[z].float()
            yout = yout.to(DEV)
        dx, grows, dg, db = _bwd_outputs(d)
        dres = torch.full_like(d.x, SENT) if residual else None
        ops.bn_bwd(dy_dev, yout, d.x, d.gamma, sm, si, dx, dg, db, nc, B, C, H * W, relu=relu,
                   dres=dres, counts=d.counts, beta=d.beta if recompute else None)
        _check_bwd(c, dx, dg, db, grows, gs, f"bn_bwd relu={relu} res={residual}")
        if residual:
            dres = dres.cpu()
            _check_rows_past_count(dres, c.counts)
            for z, n in enumerate(c.counts):
                assert torch.equal(dres[z, :n], gs[z].float()), z


@pytest.mark.parametrize("case", bn_cases.CASES, ids=case_id)
def test_bwd_tiles(case):
    """fh_bn_bwd_tiles: g already masked, the statistics from host-built tiles."""
    c = bn_cases.build(*case)
    nc, B, C, H, W = c.shape
    d = Dev(c)
    sm_ref, si_ref = d.saved_ref()
    gs = [c.dy[z, :n] * (c.y_ref(z, True, False) > 0) for z, n in enumerate(c.counts)]
    g = torch.full(c.x.shape, NAN)
    for z, n in enumerate(c.counts):
        g[z, :n] = gs[z]
    part = torch.stack([bn_ref.bwd_tiles(g[z], c.x[z], sm_ref[z], n)
                        for z, n in enumerate(c.counts)]).to(DEV)
    dx, grows, dg, db = _bwd_outputs(d)
    ops.bn_bwd_tiles(part, g.to(DEV), d.x, d.gamma, sm_ref.to(DEV), si_ref.to(DEV), dx, dg, db,
                     nc, B, C, H * W, counts=d.counts)
    _check_bwd(c, dx, dg, db, grows, gs, "bn_bwd_tiles")


@pytest.mark.parametrize("case", bn_cases.POOL_CASES, ids=case_id)
@pytest.mark.parametrize("p_drop", [0.0, 0.5])
@pytest.mark.parametrize("kind", ["pool_yout", "pool_recompute", "pool_tiles"])
def test_bwd_pool(case, p_drop, kind):
    """fh_bn_bwd_pool (ReLU mask from the stored output, or recomputed from x and beta) and
    fh_bn_bwd_pool_tiles (statistics from host-built tiles of the pooled grid): the gradient
    arrives through the 2x2 max-pool and its dropout mask."""
    c = bn_cases.build(*case)
    nc, B, C, H, W = c.shape
    d = Dev(c)
    sm_ref, si_ref = d.saved_ref()
    sm, si = sm_ref.to(DEV), si_ref.to(DEV)
    pmask = c.pmask if p_drop else None
    idx = torch.full(c.pmask.shape, 255, dtype=torch.uint8)
    yout = torch.full(c.x.shape, NAN)
    gs, keeps = [], []
    for z, n in enumerate(c.counts):
        v = c.y_ref(z, True, False)
        idx[z, :n] = bn_ref.pool_fwd(v)[1]
        yout[z, :n] = v.float()
        keeps.append(v > 0)
        routed = bn_ref.pool_route(c.dpool[z, :n], idx[z, :n],
                                   None if pmask is None else pmask[z, :n], p_drop, H, W)
        gs.append(torch.where(keeps[z], routed, torch.zeros_like(routed)))
    dq = _poison(c.dpool, c.counts).to(DEV)
    pm_dev = None if pmask is None else pmask.to(DEV)
    dx, grows, dg, db = _bwd_outputs(d)
    if kind == "pool_tiles":
        part = torch.stack([bn_ref.bwd_pool_tiles(c.dpool[z], idx[z],
                                                  None if pmask is None else pmask[z], p_drop,
                                                  c.x[z], keeps[z], sm_ref[z], n)
                            for z, n in enumerate(c.counts)]).to(DEV)
        ops.bn_bwd_pool_tiles(part, dq, idx.to(DEV), d.x, d.gamma, d.beta, sm, si, dx, dg, db,
                              nc, B, C, H, W, pmask=pm_dev, p_drop=p_drop, counts=d.counts)
    else:
        recompute = kind == "pool_recompute"
        ops.bn_bwd_pool(dq, idx.to(DEV), None if recompute else yout.to(DEV), d.x, d.gamma, sm,
                        si, dx, dg, db, nc, B, C, H, W, relu=True, pmask=pm_dev, p_drop=p_drop,
                        counts=d.counts, beta=d.beta if recompute else None)
    _check_bwd(c, dx, dg, db, grows, gs, f"{kind} p={p_drop}")


# ------------------------------------------------------------------ which branches run
def test_shapes_reach_the_slice_edges():
    """The float4 loop of the backward apply pass handles two quads of 1024 elements per
    iteration; the cases must hold slices whose last iteration has only the first quad,
    slices that end exactly on a 2048-element boundary, one that ends 4 elements past it,
    and channels split over several slices.  bn_cases.geometry restates the launch geometry
    for this assertion only; no expected value depends on it."""
    vec = [(s, n) for s, n in bn_cases.CASES if (s[3] * s[4]) % 4 == 0]
    lens = [L for s, n in vec for L in bn_cases.slice_lengths(s, n)]
    assert any(0 < L % 2048 <= 1024 for L in lens)      # ends with two == false
    assert any(L % 2048 == 0 for L in lens)             # ends on the boundary
    assert any(L % 2048 == 4 for L in lens)             # ends 4 elements past it
    assert any(1024 < L % 2048 for L in lens)           # ends with two == true, ragged
    assert any(bn_cases.geometry(s[0], s[1], s[2], s[3] * s[4])[0] > 1 for s, n in vec)
    # pooled grid: 63 / 64 / 65 tiles of 256 pooled elements, and the scalar path
    sp = {bn_ref.tiles_per_client(s[1], (s[3] // 2) * (s[4] // 2)) for s, n in bn_cases.POOL_CASES}
    assert {63, 64, 65} <= sp
    assert any(s[4] % 4 for s, n in bn_cases.POOL_CASES)
    full = {bn_ref.tiles_per_client(s[1], s[3] * s[4]) for s, n in bn_cases.CASES}
    assert {1, 63, 64, 65} <= full
