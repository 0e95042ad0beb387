"""Known-answer tests of the Philox streams: what every kernel DRAWS, element by element,
against tests/philox_ref.py (numpy, pinned to the published Random123 vectors by
tests/test_philox_ref_cpu.py, which also proves that 9 rounds, swapped counter halves, an
off-by-one counter, rotated lanes or a seed cut to 32 bits would each fail the comparisons
below).  The other suites check what is DONE with the draws (bit-exact DP with injected noise,
transforms given the recorded draws, fused == unfused masks) and their statistics; none of them
would notice a Philox with fewer rounds, aliased rows, a dropped high word, a grid-stride pass
that re-uses its counter, or a tail element with the wrong lane's draw.  Every test here
asserts on every element and launches unmodified project kernels at valid arguments.

Philox call sites in csrc/ and the test that pins each
------------------------------------------------------
`Philox::gen` has six callers:

  fh_common.h:265  gauss4                     through its two callers, below
  dp.hip:107       dp_apply_kernel            test_dp_apply_* (direct)
  fh_common.h:252  maxpool2_tail, the pool + dropout tail of two kernels:
                     maxpool2_fwd_kernel (layers.hip:63):
                                              test_maxpool_mask* (direct; dense, pitched); its
                                              BN-on-load entry (fh_maxpool2_fwd_bnrelu) is the
                                              same kernel, tied by test_fuse_bn_gpu.py::
                                              test_fused_ops_match_apply_pass (m1 == m2)
                     maxpool2_bnfin_kernel (bn.hip:320):
                                              test_fuse_bn_gpu.py::
                                              test_pool_finalize_matches_separate_launches
                                              (mask == maxpool2_fwd's), and
                                              test_fused_pool_finalize_mask[_after_split_conv]
                                              (direct, id block; after an unsplit and a split
                                              conv plan)
  layers.hip:121   dropout_fwd_kernel         test_dropout_mask* (direct)
  layers.hip:886   gather_u8_kernel           test_gather_u8_draws* (direct); the pixels are tied
                                              to the recorded draws by the oracle test
  conv.hip:71      apply_dropout, called with a counter of its own from four FWD epilogues, all
                   reached through fh_linear_fwd_dropout:
                     linear_fwd_skinny_kernel (conv.hip:3465) and linear_fwd_epilogue_kernel
                     (:3503), batch <= 32:     test_classifier_gpu.py::
                                              test_linear_fwd_dropout_equals_two_launches
                                              (mask == dropout_fwd's; its shapes all take
                                              these two), and test_fused_linear_dropout_mask
                                              [skinny, skinny_splitk] (direct, id block)
                     igemm_kernel (:448) and splitk_epilogue_kernel (:647), batch > 32 or
                     in_f % 32 != 0:           no equality test runs them;
                                              test_fused_linear_dropout_mask[igemm,
                                              igemm_splitk] (direct, id block)

`gauss4` has two callers:

  dpsgd.hip:82     dpsgd_noise_kernel         test_dpsgd_noise* (direct)
  optim.hip:174    opt_slabs_kernel<.., DP>   fh_dpsgd_step_slabs is proven bit-identical to
                                              slab_wsum + dpsgd_noise + the optimizer step by
                                              test_dpsgd_gpu.py::
                                              test_dpsgd_fused_step_bit_identical; not repeated

The equality tests of the fused sites pass no device key block, so each fused site also gets
one direct case WITH a block holding a client id >= 2^32: the key rule (seed + block[0],
philox_row) is re-implemented at every site.  Whole-network runs with client ids are
test_client_keys_gpu.py's (equal across layouts).

The Gaussian tolerance (philox_ref.GAUSS_TOL, per unit sigma)
------------------------------------------------------------
Masks and integer draws are exact.  The device evaluates Box-Muller in fp32 (the build has
-ffp-contract=off and no fast-math flag, so logf / sincosf / sqrtf are the accurate library
versions); the reference is fp64 on the same uniforms (u01 is exact in both).  With
ulp = 2^-23 (relative) and g = r cos(theta) or r sin(theta):

  |dg| <= r (|dtheta| + e_sincos) + |dr| + 2^-24 |g|
  r        <= sqrt(2 * 24 ln 2) = 5.77                 u01 >= 2^-24
  |dtheta| <= 2 pi * 2 * 2^-24 = 7.5e-7                the fp32 constant 2 pi and the rounding
                                                       of its product with u01
  e_sincos <= 4 ulp of a value <= 1 = 4.8e-7           sinf / cosf / sincosf: <= 4 ulp
  |dr| / r <= 3 ulp + 3 ulp / 2 = 5.4e-7               sqrtf <= 3 ulp; logf <= 3 ulp, halved by
                                                       the square root; the factor -2 is exact
  2^-24 |g|                                            the rounding of the product r * cos

  GAUSS_TOL = 5.77 * (7.5e-7 + 4.8e-7) + 5.77 * 5.4e-7 + 5.77 * 6.0e-8 = 1.05e-5

The 3 / 4 / 3 ulp figures are the OpenCL full-profile limits for log, sin / cos / sincos and
sqrt: limits of the OpenCL specification, not figures that ROCm publishes.  The ROCm
installation ships the device math library (OCML, lib/llvm/lib/clang/*/lib/amdgcn/bitcode/
ocml.bc) but no accuracy table for it; HIP's logf / sincosf / sqrtf compile to OCML's log /
sincos / sqrt, and that OCML (which also serves OpenCL) meets those limits is an ASSUMPTION of
this bound.  The measured errors, below, are six times smaller.  With 2 ulp each the same
formula gives about 7e-6; numpy's correctly rounded fp32 steps give 1.8e-6.

A consumer adds its own roundings: noise = fl(sigma * g) and the final add, each 2^-24 of the
value, so |out - (base + sigma g)| <= sigma GAUSS_TOL + 2^-24 (|sigma g| + |base + sigma g|).
A wrong stream errs by O(sigma): the margin is about 10^5.

Maximum error measured on the MI355X, per unit sigma (|out - ref| / sigma over every element
of every Gaussian case here): 1.66e-6 for dp_apply (the 2,098,179-element row; 1.1e-6 over the
4099-element rows) and 1.80e-6 for dpsgd_noise (its 2,098,179-element row, the rounding of the
add onto a non-zero gradient included) — 0.16 and 0.17 of the bound.
"""
import numpy as np
import pytest
import torch

import philox_ref as pr
import small_ref as sr
from fedhip import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
U = 2.0 ** -24
GUARD = 0xAB                       # fill of every uint8 output buffer: never a mask / draw value
GRID_ELEMS = 2048 * 256            # elements one pass of a capped elementwise grid covers
BIG_ID = (3 << 32) | 7             # a client id whose low word is another client's whole id
SEED_HI = (5 << 32) | 1234         # a seed whose low word is another run's whole seed
STEP_KEY = (9 << 32) | 0x11        # a device step key >= 2^32


def _block(step_key, ids=None):
    """(numpy key block, the same on the device as the int64 tensor the engine passes)."""
    blk = pr.key_block(step_key, ids)
    return blk, torch.from_numpy(blk.view(np.int64).copy()).to(DEV)


def _i32(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)


def _check_gauss(got, base, scale, g, what, extra=0.0):
    """got == base + scale * g (float64 arrays) within the Gaussian tolerance, one rounding of
    the noise product and one of the final add, plus `extra` (the consumer's other roundings)."""
    noise = scale * g
    ref = base + noise
    tol = scale * pr.GAUSS_TOL + U * (np.abs(noise) + np.abs(ref)) + extra
    err = np.abs(got - ref)
    print(f"{what}: max |err| / sigma = {err.max() / scale:.3e} (bound {pr.GAUSS_TOL:.3e}), "
          f"max err / tol = {(err / tol).max():.3f}")
    bad = np.flatnonzero(err > tol)
    assert bad.size == 0, (what, bad[:8], err[bad[:8]], tol[bad[:8]])


def _differ(a, b, scale):
    """Two streams are different draws: almost every element apart by far more than the bound."""
    return (np.abs(a - b) > 2.0 * scale * pr.GAUSS_TOL).mean() >= 0.99


# ------------------------------------------------------------------ dp_apply
def _dp_apply(P, sigmas, seed, row_ids=None, local=None, glob=None, coef=None, clipped=None):
    """out [C, P] as float64 (numpy); the padding behind every row checked untouched."""
    C = len(sigmas)
    ld = torch.zeros(C, P, device=DEV) if local is None else local.to(DEV)
    gd = None if glob is None else glob.to(DEV)
    ob, ov = sr.padded(C, P, torch.float32, DEV)
    before = ob.clone()
    cf = torch.ones(C, device=DEV) if coef is None else torch.tensor(coef, dtype=torch.float32,
                                                                    device=DEV)
    cl = _i32([0] * C if clipped is None else clipped)
    sg = torch.tensor(sigmas, dtype=torch.float32, device=DEV)
    ids = None if row_ids is None else torch.tensor(row_ids, dtype=torch.int64, device=DEV)
    ops.dp_apply(ld, gd, ov, cf, cl, sg, seed=seed, P=P, row_ids=ids)
    torch.cuda.synchronize()
    assert sr.untouched_outside(ob, before, [P] * C)
    return ov.cpu().double().numpy()


@pytest.mark.parametrize("P", [1, 5, 6, 7, 4099])
def test_dp_apply_tails_and_row_index_key(P):
    """All four P % 4 tails, three rows with their own sigma; without row_ids the key of a row
    is its index."""
    sigmas = [0.5, 2.0, 1.25]
    out = _dp_apply(P, sigmas, seed=1234)
    for z, s in enumerate(sigmas):
        _check_gauss(out[z], 0.0, s, pr.gauss_row(1234, z, P), f"dp_apply P={P} row {z}")


def test_dp_apply_second_grid_pass():
    """A row longer than the capped grid (2048 x 256 quads): the second grid-stride pass draws
    under its own counters, and the tail behind it too (CIFAR10CNN's row is this long)."""
    j0 = GRID_ELEMS * 4
    P = j0 + 1027
    out = _dp_apply(P, [1.0], seed=99, row_ids=[11])[0]
    _check_gauss(out, 0.0, 1.0, pr.gauss_row(99, 11, P), "dp_apply second pass")
    assert out[j0] != out[0]
    assert not np.array_equal(out[j0:], out[:1027])


def test_dp_apply_high_words_of_seed_and_id():
    """A seed / client id >= 2^32 next to the same low words with zero high words: four
    different streams, each the reference's."""
    P = 4099
    ids = [BIG_ID, BIG_ID & 0xFFFFFFFF]
    rows = {}
    for seed in (SEED_HI, SEED_HI & 0xFFFFFFFF):
        out = _dp_apply(P, [1.5, 1.5], seed=seed, row_ids=ids)
        for z, rid in enumerate(ids):
            _check_gauss(out[z], 0.0, 1.5, pr.gauss_row(seed, rid, P),
                         f"dp_apply seed {seed:#x} id {rid:#x}")
            rows[(seed, rid)] = out[z]
    keys = list(rows)
    assert len(keys) == 4
    for i in range(4):
        for j in range(i + 1, 4):
            assert _differ(rows[keys[i]], rows[keys[j]], 1.5), (keys[i], keys[j])


def test_dp_apply_clipped_with_global_row():
    """out = global + (delta * coef + sigma g) with a clipped and an unclipped row.  Beyond the
    Gaussian tolerance (which holds the roundings of sigma g and of the last add): the
    subtraction l - g, the product with coef (clipped row only) and the add of the noise, each
    2^-24 of its result."""
    C, P = 2, 4099
    gen = torch.Generator().manual_seed(3)
    glob = torch.randn(C, P, generator=gen)
    local = glob + 0.1 * torch.randn(C, P, generator=gen)
    coef, clipped, sigmas, ids = [0.37109375, 1.0], [1, 0], [0.75, 1.5], [BIG_ID, 4]
    out = _dp_apply(P, sigmas, seed=SEED_HI, row_ids=ids, local=local, glob=glob, coef=coef,
                    clipped=clipped)
    for z in range(C):
        g64 = glob[z].double().numpy()
        delta = local[z].double().numpy() - g64
        d = delta * coef[z] if clipped[z] else delta
        noise = sigmas[z] * pr.gauss_row(SEED_HI, ids[z], P)
        extra = U * (np.abs(delta) + (np.abs(d) if clipped[z] else 0.0) + np.abs(d + noise))
        _check_gauss(out[z], g64 + d, sigmas[z], noise / sigmas[z], f"dp_apply clipped row {z}",
                     extra=extra)


# ------------------------------------------------------------------ dpsgd_noise
def _dpsgd_noise(n, stride, batch, counts, sigma_c, seed, block):
    """grad[z][j] += fl32(sigma_c / cnt_z) * N(0, 1) for j < n on a known buffer: elements
    >= n and rows with cnt 0 keep their bits."""
    C = len(counts) if counts is not None else 3
    blk, blk_t = (None, None) if block is None else _block(*block)
    g0 = torch.randn(C, stride, generator=torch.Generator().manual_seed(n))
    grads = g0.to(DEV)
    ops.dpsgd_noise(grads, n, C, batch, sigma_c, seed=seed, seed_dev=blk_t, counts=_i32(counts))
    torch.cuda.synchronize()
    got = grads.cpu()
    eff = pr.effective_seed(seed, blk)
    noise = {}
    for z in range(C):
        cnt = batch if counts is None else counts[z]
        if cnt <= 0:
            assert sr.same_bits(got[z], g0[z]), z
            continue
        assert sr.same_bits(got[z, n:], g0[z, n:]), z
        s = float(np.float32(sigma_c) / np.float32(cnt))
        g = pr.gauss_row(eff, pr.row_key(blk, z), n)
        _check_gauss(got[z, :n].double().numpy(), g0[z, :n].double().numpy(), s, g,
                     f"dpsgd_noise n={n} row {z} cnt {cnt}")
        noise[z] = (got[z, :n].double().numpy() - g0[z, :n].double().numpy()) / s
    return noise


@pytest.mark.parametrize("n", [1025, 1026, 1027])
@pytest.mark.parametrize("form", ["no_block", "no_block_full_batches", "block_without_ids",
                                  "block_with_ids"])
def test_dpsgd_noise_key_forms(form, n):
    """The three key forms (no device block; a block without ids; a block with client ids, one
    >= 2^32), every n % 4 != 0 tail below the row stride, ragged counts with a 0: the scale is
    sigma_c / cnt of the row."""
    counts, batch = [9, 4, 0, 7], 9
    if form == "no_block":
        _dpsgd_noise(n, 1040, batch, counts, 2.5, SEED_HI, None)
    elif form == "no_block_full_batches":
        _dpsgd_noise(n, 1040, batch, None, 2.5, SEED_HI, None)
    elif form == "block_without_ids":  # seed + step key wraps mod 2^64
        _dpsgd_noise(n, 1040, batch, counts, 2.5, (1 << 64) - 3, (STEP_KEY, None))
    else:
        low = BIG_ID & 0xFFFFFFFF
        noise = _dpsgd_noise(n, 1040, batch, counts, 2.5, 77, (STEP_KEY, [low, BIG_ID, 9, 2]))
        assert _differ(noise[0], noise[1], 1.0)  # the id's high word selects another stream


def test_dpsgd_noise_second_grid_pass():
    n = GRID_ELEMS * 4 + 1027
    _dpsgd_noise(n, n + 5, 4, [3], 0.75, 5, (STEP_KEY, [BIG_ID]))


# ------------------------------------------------------------------ keep-masks
def _check_dropped(y, ref, mask, what):
    """y (fp32 tensor) == ref (fp64: the undropped value / (1 - p)) within 1 fp32 ulp where
    kept, and +0 where dropped."""
    keep = mask.astype(bool)
    yv = y.double().numpy()
    assert (np.abs(yv - ref)[keep] <= sr.ulp32(ref)[keep]).all(), what
    assert not sr.bits(y).numpy()[~keep].any(), what


def _dropout_case(B, per_img, counts, p, seed, block):
    nc, n = len(counts), B * per_img
    blk, blk_t = (None, None) if block is None else _block(*block)
    x = torch.randn(nc, n, generator=torch.Generator().manual_seed(per_img))
    yb, yv = sr.padded(nc, n, torch.float32, DEV)
    mb, mv = sr.padded(nc, n, torch.uint8, DEV, fill=GUARD, pad=7)
    yb0, mb0 = yb.clone(), mb.clone()
    ops.dropout_fwd(x.to(DEV), yv, mv, nc, B, per_img, p, drop_mode=1, seed=seed,
                    counts=_i32(counts), seed_dev=blk_t)
    torch.cuda.synchronize()
    lens = [c * per_img for c in counts]
    assert sr.untouched_outside(yb, yb0, lens) and sr.untouched_outside(mb, mb0, lens)
    eff = pr.effective_seed(seed, blk)
    y, m = yv.cpu(), mv.cpu()
    for z, k in enumerate(lens):
        want = pr.keep_mask(eff, pr.row_key(blk, z), k, p)
        assert torch.equal(m[z, :k], torch.from_numpy(want)), z
        _check_dropped(y[z, :k], x[z, :k].double().numpy() / (1.0 - p), want, z)


@pytest.mark.parametrize("p", [0.5, 0.25, 0.3])
@pytest.mark.parametrize("block", [None, (STEP_KEY, [4, BIG_ID, BIG_ID & 0xFFFFFFFF])],
                         ids=["no_block", "id_block"])
def test_dropout_mask(p, block):
    """per_img no multiple of 4, ragged counts with a 0, with and without an id block."""
    _dropout_case(6, 10, [6, 0, 3], p, SEED_HI, block)


def test_dropout_mask_past_the_grid_cap():
    """3 x 32 x 130 elements per image, 44 images: the second client's elements end inside
    the grid-stride loop's second pass."""
    per_img = 3 * 32 * 130
    assert 43 * per_img > GRID_ELEMS
    _dropout_case(44, per_img, [44, 43, 0], 0.3, 77, (STEP_KEY, [BIG_ID, 1, 2]))


def _pool_windows(x):
    """Max of every 2x2 window, [.., H, W] -> [.., H/2, W/2] (comparisons only: exact)."""
    return torch.maximum(torch.maximum(x[..., 0::2, 0::2], x[..., 0::2, 1::2]),
                         torch.maximum(x[..., 1::2, 0::2], x[..., 1::2, 1::2]))


def _maxpool_case(B, C, H, counts, p, seed, block, pitch=None):
    """The counter of a keep decision is the dense pooled element index e, whatever the plane
    pitch; nothing past a client's images (or outside the embedded map) is written."""
    nc, OH = len(counts), H // 2
    per = C * OH * OH
    blk, blk_t = (None, None) if block is None else _block(*block)
    x = torch.randn(nc, B, C, H, H, generator=torch.Generator().manual_seed(H * C))
    if pitch:
        xd = torch.full((nc, B, C, pitch, pitch), 7.0, device=DEV)
        xd[..., :H, :H] = x.to(DEV)
        yb = torch.full((nc, B + 1, C, pitch, pitch), sr.SENTINEL, device=DEV)
    else:
        xd = x.to(DEV)
        yb = torch.full((nc, B + 1, C, OH, OH), sr.SENTINEL, device=DEV)
    ib = torch.full((nc, B + 1, C, OH, OH), GUARD, dtype=torch.uint8, device=DEV)
    mb = torch.full((nc, B + 1, C, OH, OH), GUARD, dtype=torch.uint8, device=DEV)
    yb0 = yb.clone()
    ops.maxpool2_fwd(xd, yb[:, :B], ib[:, :B], nc, B, C, H, H, mask=mb[:, :B], drop_mode=1,
                     p_drop=p, seed=seed, counts=_i32(counts), seed_dev=blk_t)
    torch.cuda.synchronize()
    lens = [c * per for c in counts]
    guard = torch.full_like(mb, GUARD).view(nc, -1)
    assert sr.untouched_outside(mb.view(nc, -1), guard, lens)
    assert sr.untouched_outside(ib.view(nc, -1), guard, lens)
    y, m = yb.cpu(), mb.cpu()
    eff = pr.effective_seed(seed, blk)
    pooled = _pool_windows(x).double()
    for z, c in enumerate(counts):
        want = pr.keep_mask(eff, pr.row_key(blk, z), lens[z], p)
        assert torch.equal(m[z, :c].reshape(-1), torch.from_numpy(want)), z
        _check_dropped(y[z, :c, :, :OH, :OH].reshape(-1),
                       pooled[z, :c].reshape(-1).numpy() / (1.0 - p), want, z)
        assert sr.same_bits(y[z, c:], yb0[z, c:].cpu()), z
    if pitch:
        assert bool((y[..., OH:] == sr.SENTINEL).all() and (y[..., OH:, :] == sr.SENTINEL).all())


@pytest.mark.parametrize("H", [4, 14, 32])
@pytest.mark.parametrize("C", [3, 32])
def test_maxpool_mask(C, H):
    """Every map size with 3 and 32 channels, ragged counts with a 0; the 32 x 32 x 32 case
    has 65 images: more pooled elements than the capped grid covers in one pass."""
    block = (STEP_KEY, [BIG_ID, 6, BIG_ID & 0xFFFFFFFF]) if C == 32 else None
    B = 65 if (C, H) == (32, 32) else 5
    if B == 65:
        assert B * C * (H // 2) ** 2 > GRID_ELEMS
    _maxpool_case(B, C, H, [B, 3, 0], 0.3, SEED_HI, block)


def test_maxpool_mask_pitched():
    """14 x 14 maps in 16 x 16 planes (test_layers_gpu.py::test_pitched_maxpool_matches_dense's
    layout): the counter stays the dense index."""
    _maxpool_case(5, 32, 14, [5, 2, 0], 0.25, 77, (STEP_KEY, [1, BIG_ID, 2]), pitch=16)


# ------------------------------------------------------------------ fused dropout sites
def _ragged(nc, B, seed):
    g = torch.Generator().manual_seed(seed)
    return [B] + [int(v) for v in torch.randint(1, B + 1, (nc - 1,), generator=g)]


def _ids(nc):
    return [BIG_ID + z if z % 2 == 0 else z for z in range(nc)]


def _check_mask_rows(mb, counts, per, p, seed, blk):
    """mb: uint8 [nc, B + 1, ...] filled with GUARD before the launch that wrote [:, :B]."""
    nc = len(counts)
    lens = [c * per for c in counts]
    assert sr.untouched_outside(mb.view(nc, -1), torch.full_like(mb, GUARD).view(nc, -1), lens)
    m = mb.cpu().view(nc, -1)
    eff = pr.effective_seed(seed, blk)
    for z, k in enumerate(lens):
        want = pr.keep_mask(eff, pr.row_key(blk, z), k, p)
        assert torch.equal(m[z, :k], torch.from_numpy(want)), z


# fh_linear_fwd_dropout's four epilogues (the launched kernels confirmed once with a kernel trace):
#   B <= 32 and in_f % 32 == 0: linear_fwd_skinny_kernel's own epilogue (9 clients: one k-chunk),
#     or linear_fwd_epilogue_kernel (1 client, K = 2048: four k-chunks);
#   otherwise run_mn<OP_FWD>: igemm_kernel's epilogue (K = 96 cannot split: fewer than four 16-k
#     steps per split), or splitk_epilogue_kernel (1 client, K = 2048: 4 tiles < 192, 32 splits).
LINEAR_CASES = [(9, 32, 128, 64), (1, 32, 2048, 512), (3, 33, 96, 80), (1, 64, 2048, 512)]


@pytest.mark.parametrize("nc,B,in_f,out_f", LINEAR_CASES,
                         ids=["skinny", "skinny_splitk", "igemm", "igemm_splitk"])
def test_fused_linear_dropout_mask(nc, B, in_f, out_f):
    """fh_linear_fwd_dropout's epilogue draw (conv.hip apply_dropout) in each of the four kernels
    that make it, under a key block with client ids and ragged counts: the mask is the
    reference's under counter img * out_f + o; y is +0 where dropped and relu(x w^T + b) / (1 - p)
    where kept (fp64, within the dot product's rounding bound (K + 4) 2^-24 (|x| |w|^T + |b|),
    any summation order); nothing is written past a client's images."""
    p = 0.3
    counts = _ragged(nc, B, in_f)
    blk, blk_t = _block(STEP_KEY, _ids(nc))
    g = torch.Generator(device=DEV).manual_seed(nc + in_f)
    x = torch.randn(nc, B, in_f, generator=g, device=DEV)
    w = torch.randn(nc, out_f, in_f, generator=g, device=DEV) * 0.05
    b = torch.randn(nc, out_f, generator=g, device=DEV) * 0.1
    eb = torch.full((nc, B + 1, out_f), sr.SENTINEL, device=DEV)
    eb0 = eb.clone()
    mb = torch.full((nc, B + 1, out_f), GUARD, dtype=torch.uint8, device=DEV)
    ops.linear_fwd_dropout(x, w, b, eb[:, :B], mb[:, :B], nc, B, in_f, out_f, p, drop_mode=1,
                           seed=77, counts=_i32(counts), seed_dev=blk_t)
    torch.cuda.synchronize()
    _check_mask_rows(mb, counts, out_f, p, 77, blk)
    assert sr.untouched_outside(eb.view(nc, -1), eb0.view(nc, -1), [c * out_f for c in counts])
    xc, wc, bc, y, m = x.cpu().double(), w.cpu().double(), b.cpu().double(), eb.cpu(), mb.cpu()
    for z, c in enumerate(counts):
        pre = xc[z, :c] @ wc[z].T + bc[z]
        bound = (in_f + 4) * U * (xc[z, :c].abs() @ wc[z].abs().T + bc[z].abs()) / (1.0 - p)
        keep = m[z, :c].bool()
        assert not sr.bits(y[z, :c])[~keep].any(), z
        err = (y[z, :c].double() - pre.clamp(min=0.0) / (1.0 - p)).abs()
        assert bool((err[keep] <= bound[keep]).all()), (z, float((err / bound)[keep].max()))


def _conv_with_stats(nc, B, ci, co, hw, cd, in_affine=False):
    """in_affine: the input is a BN pre-activation, relu(x*scale + shift) applied on load."""
    torch.manual_seed(nc * 11 + co)
    x = torch.randn(nc, B, ci, hw, hw, device=DEV)
    w = torch.randn(nc, co, ci, 3, 3, device=DEV) / (3.0 * ci ** 0.5)
    bias = torch.randn(nc, co, device=DEV) * 0.2
    c = torch.zeros(nc, B, co, hw, hw, device=DEV)
    part = torch.zeros(nc, co, ops.bnstats_tiles(B, hw, hw), 2, dtype=torch.float64, device=DEV)
    aff = None
    if in_affine:
        aff = (torch.rand(nc, ci, device=DEV) + 0.5, torch.randn(nc, ci, device=DEV) * 0.1)
    ops.conv2d_fwd(x, w, bias, c, nc, B, ci, hw, hw, co, 3, 1, 1, counts=cd, in_affine=aff,
                   bn_stats=part)
    return c, part


def _pool_finalize(nc, B, C, hw, cd, c, part, p, seed, blk_t):
    gamma = torch.rand(nc, C, device=DEV) + 0.5
    beta = torch.randn(nc, C, device=DEV) * 0.3
    rm, rv = torch.zeros(nc, C, device=DEV), torch.ones(nc, C, device=DEV)
    sm, si, sc, sh = (torch.zeros(nc, C, device=DEV) for _ in range(4))
    q = torch.zeros(nc, B, C, hw // 2, hw // 2, device=DEV)
    idx = torch.zeros(nc, B, C, hw // 2, hw // 2, dtype=torch.uint8, device=DEV)
    mb = torch.full((nc, B + 1, C, hw // 2, hw // 2), GUARD, dtype=torch.uint8, device=DEV)
    ops.maxpool2_fwd_bnfinalize(part, gamma, beta, rm, rv, sm, si, sc, sh, c, q, idx, nc, B, C, hw,
                                hw, mask=mb[:, :B], drop_mode=1, p_drop=p, seed=seed, counts=cd,
                                seed_dev=blk_t)
    torch.cuda.synchronize()
    return mb


def test_fused_pool_finalize_mask():
    """maxpool2_bnfin_kernel's draw (fh_maxpool2_fwd_bnfinalize after an unsplit conv) under a
    key block with client ids."""
    nc, B, C, hw, p = 3, 32, 128, 8, 0.3
    counts = _ragged(nc, B, C)
    blk, blk_t = _block(STEP_KEY, _ids(nc))
    cd = _i32(counts)
    c, part = _conv_with_stats(nc, B, 16, C, hw, cd)
    mb = _pool_finalize(nc, B, C, hw, cd, c, part, p, 5, blk_t)
    _check_mask_rows(mb, counts, C * (hw // 2) ** 2, p, 5, blk)


def test_fused_pool_finalize_mask_after_split_conv():
    """maxpool2_bnfin_kernel's draw after a conv that takes a split plan (one client on the
    whole chip: the statistics tiles come from the split reduction's epilogue), its input a BN
    pre-activation, under a key block with a client id >= 2^32."""
    nc, B, C, hw, p = 1, 32, 64, 16, 0.3
    ops.set_fill_fraction(1.0)  # the split plan assumes the whole-chip planner
    counts = [B]
    cd = _i32(counts)
    blk, blk_t = _block(STEP_KEY, [BIG_ID])
    c, part = _conv_with_stats(nc, B, 64, C, hw, cd, in_affine=True)
    mb = _pool_finalize(nc, B, C, hw, cd, c, part, p, 17, blk_t)
    _check_mask_rows(mb, counts, C * (hw // 2) ** 2, p, 17, blk)


# ------------------------------------------------------------------ crop / flip draws
def _gather_u8(tf, shape, counts, seed, block):
    S, B, N = len(counts), 32, 40
    blk, blk_t = (None, None) if block is None else _block(*block)
    g = torch.Generator().manual_seed(8)
    data = torch.randint(0, 256, (N,) + shape, generator=g, dtype=torch.uint8).to(DEV)
    labels = torch.randint(0, 10, (N,), generator=g).to(DEV)
    idx = torch.randint(0, N, (S, B), generator=g).to(DEV)
    E = int(np.prod(shape))
    x = torch.zeros(S, B * E, device=DEV)
    y = torch.zeros(S, B, dtype=torch.int64, device=DEV)
    aug = torch.full((S, B, 4), GUARD, dtype=torch.uint8, device=DEV)
    ops.gather_u8(data, labels, idx, x, y, tf, S, B, counts=_i32(counts), seed=seed,
                  seed_dev=blk_t, aug_out=aug)
    torch.cuda.synchronize()
    return aug.cpu(), blk


@pytest.mark.parametrize("block", [None, (STEP_KEY, [BIG_ID & 0xFFFFFFFF, BIG_ID, 5])],
                         ids=["no_block", "id_block"])
def test_gather_u8_draws(block):
    """RandomCrop(32, 4) + RandomHorizontalFlip: the recorded (i, j, flip) of batch slot b is
    the reference's draw under counter b, for every valid slot; nothing is recorded beyond."""
    counts = [32, 17, 0]
    aug, blk = _gather_u8(ops.DataTransform.cifar10(train=True), (32, 32, 3), counts, SEED_HI,
                          block)
    eff = pr.effective_seed(SEED_HI, blk)
    for z, c in enumerate(counts):
        want = pr.crop_flip(eff, pr.row_key(blk, z), np.arange(c), 4)
        assert torch.equal(aug[z, :c, :3], torch.from_numpy(want).view(c, 3)), z
        assert not aug[z, :c, 3].any()
        assert bool((aug[z, c:] == GUARD).all()), z
    if block is not None:  # the id's high word selects another stream
        assert not torch.equal(aug[0, :17, :3], aug[1, :17, :3])


def test_gather_u8_mnist_draws_nothing():
    """No padding and no flip: no draw is made and none is recorded."""
    aug, _ = _gather_u8(ops.DataTransform.mnist(), (28, 28), [32, 17, 0], SEED_HI, None)
    assert bool((aug == GUARD).all())
