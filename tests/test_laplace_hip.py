"""The fused Laplace kernels (laplace.hip) against fp64 oracles, per expert and
per gradient component, at the shapes and states where the kernel takes a
path of its own: partial Cholesky blocks, k and d that are no multiple of 4,
one to three column chunks, the LDS edge, warm and adversarial starts,
one-class experts, a broken expert inside a batch, a signed ARD scale.

Inputs are drawn in fp32 and the oracles get ``.double()`` copies of the very
same values, so a difference is the kernel's arithmetic, not input rounding.

No bound here is a number read off the kernel.  Every bound is scaled by
what plain fp32 arithmetic does on the same inputs: the same oracle is
evaluated in float32 on the CPU, its error against the fp64 result is
measured per expert and per group as

    max|x - x64| / max(max|x64|, 1)

and the kernel passes with an error of at most ``max(FACTOR * fp32 error,
floor)``.  FACTOR = 8 covers what the kernel does beyond a plain fp32
evaluation (``__expf`` and the fast sigmoid, the explicit inverse V in place
of triangular solves, the fp32 ``z * z`` atomics of diagKRK).

The reference builders below run on the CPU alone; tests/test_classification.py
pins them against the generic Laplace path on machines without a GPU.
"""

import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TD = torch.float64
FACTOR = 8.0
FLOOR_EVIDENCE = 1e-5     # evidence groups (relative measure above)
FLOOR_STEP = 1e-5         # one- and two-step latent (relative measure above)
FLOOR_MODE = 1e-4         # converged latent, absolute: sqrt(tol)-scale slack
                          # of the |delta psi| <= tol stop at tol = 1e-6
TOL = 1e-6                # == hip_backend.LAPLACE_MIN_TOL
GROUPS = ("logZ", "scale", "amp", "noise")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from spark_gp_amd import _hip_ext
    return _hip_ext


# ---------------------------------------------------------------------------
# inputs (CPU only)
# ---------------------------------------------------------------------------

def ard_scale(d, g):
    """Unequal fp32 entries with magnitudes in [0.3, 2.5], one of them
    negative.  The upper end shrinks with d so that q = ||(a - b) o s||^2
    stays O(1) on U[0,1)^d and the base kernel is not numerically diagonal."""
    hi = min(2.5, 0.3 + 4.0 / math.sqrt(d))
    s = (0.3 + (hi - 0.3) * torch.rand(d, generator=g)).float()
    s[d // 2] = -s[d // 2]
    return s


def rbf_scale(d):
    """The isotropic base: every entry equal (q about 2/3 on U[0,1)^d)."""
    return torch.full((d,), 2.0 / math.sqrt(d)).float()


def make_tree(base, d, scale32, amp, noise):
    """(kernel, cs, theta) of  amp * base + noise * I  with amplitude, base
    hypers and noise all trainable, such that the canonical form hands the
    kernels exactly the fp32 ``scale32``, amp and noise given here."""
    from spark_gp_amd.kernels import (ARDRBFKernel, RBFKernel,
                                      WhiteNoiseKernel, compile_kernel)
    from spark_gp_amd.kernels.compiled import base_scale
    amp, noise = float(np.float32(amp)), float(np.float32(noise))
    s32 = scale32.numpy()
    if base == "ard":
        kern = 1 * ARDRBFKernel(d) + WhiteNoiseKernel(noise, 0, 1)
        theta = np.concatenate([[amp], s32.astype(np.float64), [noise]])
    else:
        length = 1.0 / (math.sqrt(2.0) * float(s32[0]))
        kern = 1 * RBFKernel(length) + WhiteNoiseKernel(noise, 0, 1)
        theta = np.array([amp, length, noise])
    cs = compile_kernel(kern)
    assert cs is not None and cs.base == base
    s = base_scale(cs.base, theta[cs.base_idx], d)
    # what hip_backend casts to fp32 is bit for bit the scale of the test,
    # and the fp64 oracle's scale is that value to fp64 rounding
    assert (s.astype(np.float32) == s32).all()
    assert np.abs(s - s32).max() <= 1e-15 * np.abs(s32).max()
    assert cs.amp(theta) == amp and cs.noise(theta) == noise
    return kern, cs, theta


def make_inputs(E, k, d, base, amp, noise, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(E, k, d, generator=g)
    y = (X.sum(-1) > d / 2).to(torch.float32)
    scale = ard_scale(d, g) if base == "ard" else rbf_scale(d)
    kern, cs, theta = make_tree(base, d, scale, amp, noise)
    return SimpleNamespace(
        E=E, k=k, d=d, base=base, X=X, y=y, scale=scale, g=g,
        amp=float(np.float32(amp)), noise=float(np.float32(noise)),
        kern=kern, cs=cs, theta=theta, X64=X.double(), y64=y.double())


def fp64_mode(c, y64=None):
    """The fp64 posterior mode f* [E, k] (cold start, tol = 1e-12)."""
    from spark_gp_amd.ops import torch_backend as tb
    y64 = c.y64 if y64 is None else y64
    f = torch.zeros(c.E, c.k, dtype=TD)
    tb.laplace_nll_grad(c.kern, c.theta, c.X64, y64, f, 1e-12)
    assert torch.isfinite(f).all()
    return f


def evidence_groups(c, logz, g):
    """(logZ [E], g [E, d + 2]) as per-expert groups, each [E, n] fp64: logZ,
    then the gradient over the base hypers (``cs.assemble_grad``: the d
    scales of the ARD base, the one length of the isotropic base), the
    amplitude and the noise."""
    logz = logz.detach().double().cpu()
    g = g.detach().double().cpu().numpy()
    d, cs = c.d, c.cs
    rows = [cs.assemble_grad(c.theta, ge[:d], float(ge[d]), float(ge[d + 1]))
            for ge in g]
    out = torch.as_tensor(np.stack(rows))
    return {"logZ": logz.unsqueeze(-1),
            "scale": out[:, cs.base_idx],
            "amp": out[:, cs.amp_idx].unsqueeze(-1),
            "noise": out[:, cs.noise_idx[0]].unsqueeze(-1)}


def evidence_refs(c, f32, y32=None, rows=None):
    """fp64 oracle and fp32 reference of Algorithm 5.1 at the fp32 latent
    ``f32``, both as evidence_groups; checked finite."""
    from spark_gp_amd.ops import torch_backend as tb
    X, y = c.X, (c.y if y32 is None else y32)
    if rows is not None:
        X, y, f32 = X[rows], y[rows], f32[rows]
    r64 = evidence_groups(c, *tb.laplace_evidence_experts(
        c.cs, c.theta, X.double(), y.double(), f32.double()))
    r32 = evidence_groups(c, *tb.laplace_evidence_experts(
        c.cs, c.theta, X, y, f32))
    for r in (r64, r32):
        for name in GROUPS:
            assert torch.isfinite(r[name]).all(), name
    return r64, r32


def newton_steps(X, y, f, scale, amp, noise, nsteps):
    """``nsteps`` iterations of R&W Algorithm 3.1 with the full step,
    f' = K a, written out in the dtype of ``X``.  The first two candidates of
    the loop are always accepted (the objective is compared with -inf, then
    with -DBL_MAX), so this is what a Newton loop capped at one or two
    iterations must return."""
    k = X.shape[-2]
    Xs = X * scale.to(X.dtype)
    diff = Xs.unsqueeze(-2) - Xs.unsqueeze(-3)
    eye = torch.eye(k, dtype=X.dtype)
    K = amp * torch.exp(-(diff * diff).sum(-1)) + noise * eye
    f = f.clone()
    for _ in range(nsteps):
        pi = torch.sigmoid(f)
        w = pi * (1.0 - pi)
        sqw = torch.sqrt(w)
        B = eye + sqw.unsqueeze(-1) * K * sqw.unsqueeze(-2)
        L = torch.linalg.cholesky(B)
        b = w * f + (y - pi)
        Kb = (K @ b.unsqueeze(-1)).squeeze(-1)
        t = torch.cholesky_solve((sqw * Kb).unsqueeze(-1), L).squeeze(-1)
        a = b - sqw * t
        f = (K @ a.unsqueeze(-1)).squeeze(-1)
    assert torch.isfinite(f).all()
    return f


# ---------------------------------------------------------------------------
# error measure and bound
# ---------------------------------------------------------------------------

def rel_err(x, x64):
    """per expert: max|x - x64| / max(max|x64|, 1) over the last axis"""
    x, x64 = x.double().cpu(), x64.double().cpu()
    return ((x - x64).abs().amax(-1)
            / x64.abs().amax(-1).clamp_min(1.0))


def abs_err(x, x64):
    return (x.double().cpu() - x64.double().cpu()).abs().amax(-1)


def check_scaled(what, name, err_kernel, err_fp32, floor, fails):
    """kernel error <= max(FACTOR * fp32 reference error, floor), per expert;
    prints every figure before judging."""
    for e in range(err_kernel.shape[0]):
        ek, e32 = float(err_kernel[e]), float(err_fp32[e])
        bound = max(FACTOR * e32, floor)
        print(f"RATIO {what} {name} e={e} kernel={ek:.3e} fp32={e32:.3e} "
              f"ratio={ek / max(e32, 1e-300):.2f} bound={bound:.3e}")
        if not ek <= bound:
            fails.append(f"{what} {name} expert {e}: kernel error {ek:.3e} "
                         f"> bound {bound:.3e} (fp32 reference {e32:.3e})")


def check_evidence(what, got, r64, r32, fails):
    for name in GROUPS:
        check_scaled(what, name, rel_err(got[name], r64[name]),
                     rel_err(r32[name], r64[name]), FLOOR_EVIDENCE, fails)


def run_kernel(entry, c, dev, f32, tol, max_newton, y32=None, rows=None):
    """One launch of ``ext.fused_laplace_{evidence,newton}`` on (a subset of)
    the experts of ``c``; everything back on the CPU, f last."""
    X, y = c.X, (c.y if y32 is None else y32)
    if rows is not None:
        X, y, f32 = X[rows], y[rows], f32[rows]
    f = f32.clone().contiguous().to(dev)
    out = entry(X.contiguous().to(dev), y.contiguous().to(dev), f,
                c.scale.to(dev), c.amp, c.noise, tol, max_newton)
    torch.cuda.synchronize()
    return [o.cpu() for o in out] + [f.cpu()]


# ---------------------------------------------------------------------------
# 1. the evidence tail in isolation: max_newton = 0 evaluates Algorithm 5.1
#    at the given latent, converged or not
# ---------------------------------------------------------------------------

# (k, d): (base, amp, noise) and what the shape reaches
EVIDENCE_CASES = {
    (7, 3): ("ard", 1.0, 1e-2),       # k < 8; d < 4
    (31, 4): ("rbf", 0.3, 0.5),       # single Cholesky block
    (33, 5): ("ard", 30.0, 1e-3),     # one-row trailing Cholesky block
    (64, 6): ("rbf", 2.0, 1e-3),      # d + 2 = 8
    (65, 7): ("ard", 0.3, 1e-2),      # d + 2 = 9
    (100, 17): ("ard", 1.3, 0.5),     # three column chunks; W chunks 8, 8, 1
    (128, 32): ("rbf", 30.0, 1e-2),   # k = 128
    (128, 128): ("ard", 5.0, 1e-3),   # the LDS edge
}


@functools.lru_cache(maxsize=None)
def evidence_case(k, d, base=None):
    """Inputs, the two latents and their references for one shape.  ``base``
    overrides the table's (the CPU tests run every shape on both bases)."""
    tbase, amp, noise = EVIDENCE_CASES[(k, d)]
    base = base or tbase
    c = make_inputs(4 if k == 128 else 5, k, d, base, amp, noise,
                    seed=1000 * k + d)
    c.latents = {
        "unconverged": (0.7 * torch.randn(c.E, k, generator=c.g)).float(),
        "mode": fp64_mode(c).float(),
    }
    c.refs = {name: evidence_refs(c, f) for name, f in c.latents.items()}
    return c


@pytest.mark.parametrize("k,d", list(EVIDENCE_CASES))
def test_evidence_tail_vs_oracle(dev, ext, k, d):
    """``fused_laplace_evidence`` with max_newton = 0 against
    ``laplace_evidence_experts`` in fp64 at the same latent: logZ and the
    three gradient groups per expert, no convergence path in between."""
    assert ext.fused_laplace_evidence_supported(k, d)
    c = evidence_case(k, d)
    fails = []
    for name, f32 in c.latents.items():
        logz, grad, iters, bad, f_out = run_kernel(
            ext.fused_laplace_evidence, c, dev, f32, TOL, 0)
        assert (bad == 0).all(), bad
        assert (iters == 0).all(), iters
        assert torch.equal(f_out.view(torch.int32), f32.view(torch.int32)), \
            "max_newton = 0 must leave the latent bitwise alone"
        r64, r32 = c.refs[name]
        check_evidence(f"tail k={k} d={d} {c.base} {name}",
                       evidence_groups(c, logz, grad), r64, r32, fails)
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------
# 2. the Newton loop
# ---------------------------------------------------------------------------

STEP_CASES = {(13, 5): (1.0, 1e-2), (33, 5): (3.0, 1e-3),
              (100, 8): (0.5, 0.1)}            # (k, d): (amp, noise), ARD


@functools.lru_cache(maxsize=None)
def step_case(k, d, start):
    amp, noise = STEP_CASES[(k, d)]
    c = make_inputs(4, k, d, "ard", amp, noise, seed=2000 * k + d)
    c.f0 = (torch.zeros(c.E, k) if start == "zero"
            else torch.randn(c.E, k, generator=c.g).float())
    c.f64 = {n: newton_steps(c.X64, c.y64, c.f0.double(), c.scale.double(),
                             c.amp, c.noise, n) for n in (1, 2)}
    c.f32 = {n: newton_steps(c.X, c.y, c.f0, c.scale, c.amp, c.noise, n)
             for n in (1, 2)}
    return c


@pytest.mark.parametrize("start", ["zero", "warm"])
@pytest.mark.parametrize("cap", [1, 2])
@pytest.mark.parametrize("k,d", list(STEP_CASES))
def test_newton_capped_steps(dev, ext, k, d, cap, start):
    """max_newton = 1 and 2: the loop stops where it is told to, reports
    that stop, and returns one or two full Newton steps, per element."""
    c = step_case(k, d, start)
    psi, sll, iters, bad, f_out = run_kernel(
        ext.fused_laplace_newton, c, dev, c.f0, TOL, cap)
    assert (bad == 0).all(), bad
    assert (iters == cap).all(), iters
    fails = []
    check_scaled(f"steps k={k} d={d} cap={cap} {start}", "f",
                 rel_err(f_out, c.f64[cap]), rel_err(c.f32[cap], c.f64[cap]),
                 FLOOR_STEP, fails)
    assert not fails, "\n".join(fails)


# (k, d): (base, amp, noise)
CONVERGE_CASES = {(24, 7): ("ard", 1.0, 1e-2), (65, 7): ("ard", 3.0, 1e-3),
                  (100, 17): ("ard", 0.5, 0.1), (128, 32): ("rbf", 1.5, 1e-2)}
STARTS = ("cold", "warm", "mode", "opposed")


@functools.lru_cache(maxsize=None)
def converge_case(k, d):
    """Five experts: two balanced, one all ones, one all zeros, one with a
    single positive; the fp64 mode and the fp64 evidence at it."""
    from spark_gp_amd.ops import torch_backend as tb
    base, amp, noise = CONVERGE_CASES[(k, d)]
    c = make_inputs(5, k, d, base, amp, noise, seed=3000 * k + d)
    y = c.y.clone()
    y[2] = 1.0
    y[3] = 0.0
    y[4] = 0.0
    y[4, k // 2] = 1.0
    c.y, c.y64 = y, y.double()
    c.fstar = fp64_mode(c)
    c.ev64 = evidence_groups(c, *tb.laplace_evidence_experts(
        c.cs, c.theta, c.X64, c.y64, c.fstar))
    c.starts = {
        "cold": torch.zeros(c.E, k),
        "warm": (c.fstar + 0.3 * torch.randn(c.E, k, generator=c.g,
                                             dtype=TD)).float(),
        "mode": c.fstar.float(),
        "opposed": -4.0 * (2.0 * y - 1.0),
    }
    return c


@functools.lru_cache(maxsize=None)
def converge_fp32(k, d, start):
    """The fp32 reference of the whole path: the generic Newton loop in
    float32 from the same start (tol 1e-6, 40 iterations at most), then
    Algorithm 5.1 in float32 at the latent it reached."""
    from spark_gp_amd.ops import torch_backend as tb
    c = converge_case(k, d)
    f = c.starts[start].clone()
    tb.laplace_nll_grad(c.kern, c.theta, c.X, c.y, f, TOL, max_newton_iter=40)
    assert torch.isfinite(f).all()
    ev = evidence_groups(c, *tb.laplace_evidence_experts(
        c.cs, c.theta, c.X, c.y, f))
    for name in GROUPS:
        assert torch.isfinite(ev[name]).all(), name
    return f, ev


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("k,d", list(CONVERGE_CASES))
def test_newton_converges_to_fp64_mode(dev, ext, k, d, start):
    """max_newton = 40, tol = 1e-6, from a cold, a warm, an exact and an
    adversarial start, with one-class experts in the batch: the latent
    reaches the fp64 mode and the fused evidence there matches the oracle
    evidence at the mode, per expert."""
    c = converge_case(k, d)
    f32ref, ev32 = converge_fp32(k, d, start)
    f0 = c.starts[start]
    psi, sll, iters, bad, f_out = run_kernel(
        ext.fused_laplace_newton, c, dev, f0, TOL, 40)
    assert (bad == 0).all(), bad
    assert ((iters >= 1) & (iters <= 40)).all(), iters
    print(f"ITERS k={k} d={d} {start}: {iters.tolist()}")
    fails = []
    what = f"converge k={k} d={d} {c.base} {start}"
    check_scaled(what, "f", abs_err(f_out, c.fstar),
                 abs_err(f32ref, c.fstar), FLOOR_MODE, fails)
    # the evidence entry point runs the same loop, then the tail
    logz, grad, iters_ev, bad_ev, f_ev = run_kernel(
        ext.fused_laplace_evidence, c, dev, f0, TOL, 40)
    assert (bad_ev == 0).all(), bad_ev
    assert torch.equal(iters_ev, iters)
    assert torch.equal(f_ev.view(torch.int32), f_out.view(torch.int32))
    check_evidence(what, evidence_groups(c, logz, grad), c.ev64, ev32, fails)
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------
# 3. breakdown inside a batch
# ---------------------------------------------------------------------------

def test_breakdown_inside_batch(dev, ext):
    """One expert of five holds a single inf in X.  It is flagged bad = 2,
    its outputs are zeroed and its latent left alone; its neighbours come
    out as if it were not there."""
    from spark_gp_amd.ops import hip_backend
    k, d, broken = 33, 5, 2
    c = make_inputs(5, k, d, "ard", 1.0, 1e-2, seed=77)
    c.X[broken, 4, 1] = float("inf")
    good = [e for e in range(c.E) if e != broken]
    f0 = (0.7 * torch.randn(c.E, k, generator=c.g)).float()

    # evidence tail at the given latent
    logz, grad, iters, bad, f_out = run_kernel(
        ext.fused_laplace_evidence, c, dev, f0, TOL, 0)
    assert bad.tolist() == [2 if e == broken else 0 for e in range(c.E)]
    assert (grad[broken] == 0).all(), grad[broken]
    assert float(logz[broken]) == 0.0
    assert (iters == 0).all(), iters
    assert torch.equal(f_out.view(torch.int32), f0.view(torch.int32))
    r64, r32 = evidence_refs(c, f0, rows=good)
    fails = []
    check_evidence("breakdown tail", evidence_groups(c, logz[good], grad[good]),
                   r64, r32, fails)
    assert not fails, "\n".join(fails)

    # full evidence launch: the broken expert never starts iterating
    logz, grad, iters, bad, f_ev = run_kernel(
        ext.fused_laplace_evidence, c, dev, f0, TOL, 40)
    assert bad.tolist() == [2 if e == broken else 0 for e in range(c.E)]
    assert (grad[broken] == 0).all() and float(logz[broken]) == 0.0
    assert int(iters[broken]) == 0
    assert torch.equal(f_ev[broken].view(torch.int32),
                       f0[broken].view(torch.int32))
    assert torch.isfinite(grad).all() and torch.isfinite(logz).all()

    # Newton-only entry point; the neighbours equal a launch without it
    psi, sll, iters_n, bad_n, f_n = run_kernel(
        ext.fused_laplace_newton, c, dev, f0, TOL, 40)
    assert bad_n.tolist() == [2 if e == broken else 0 for e in range(c.E)]
    assert int(iters_n[broken]) == 0
    assert torch.equal(f_n[broken].view(torch.int32),
                       f0[broken].view(torch.int32))
    psi_g, _, iters_g, bad_g, f_g = run_kernel(
        ext.fused_laplace_newton, c, dev, f0, TOL, 40, rows=good)
    assert (bad_g == 0).all() and (iters_g >= 1).all()
    assert torch.equal(f_n[good].view(torch.int32), f_g.view(torch.int32))
    assert torch.equal(iters_n[good], iters_g)
    assert torch.equal(psi[good].view(torch.int64), psi_g.view(torch.int64))
    assert torch.equal(f_ev[good].view(torch.int32), f_g.view(torch.int32))

    # host level: the count of bad experts, and None for the evidence
    Xd, yd = c.X.to(dev), c.y.to(dev)
    f1 = f0.clone().to(dev)
    assert hip_backend.laplace_newton(c.cs, c.theta, Xd, yd, f1, TOL, 40) == 1
    f2 = f0.clone().to(dev)
    assert hip_backend.laplace_evidence(c.cs, c.theta, Xd, yd, f2, TOL,
                                        40) is None


# ---------------------------------------------------------------------------
# 4. independence and determinism
# ---------------------------------------------------------------------------

def test_experts_independent_and_deterministic(dev, ext):
    """Six differing experts at (65, 7): each comes out of the batch exactly
    as it does launched alone, and a repeated launch repeats.  The Newton
    loop has no atomics and block_sum a fixed order, so f, psi and iters are
    bitwise; so is logZ.  The gradient passes through the LDS-atomic
    diagKRK, whose order varies: relative 1e-6."""
    k, d = 65, 7
    c = make_inputs(6, k, d, "ard", 1.0, 1e-2, seed=99)
    f0 = (0.5 * torch.randn(c.E, k, generator=c.g)).float()

    def same_bits(a, b):
        assert a.dtype == b.dtype and a.shape == b.shape
        return torch.equal(a.reshape(-1).view(torch.uint8),
                           b.reshape(-1).view(torch.uint8))

    def grads_close(a, b):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-6,
                                   atol=1e-6 * float(b.abs().max()))

    psi, sll, iters, bad, f = run_kernel(
        ext.fused_laplace_newton, c, dev, f0, TOL, 40)
    assert (bad == 0).all() and (iters >= 1).all()
    logz, grad, iters_ev, bad_ev, f_ev = run_kernel(
        ext.fused_laplace_evidence, c, dev, f0, TOL, 40)
    assert (bad_ev == 0).all()
    assert same_bits(f_ev, f) and same_bits(iters_ev, iters)

    psi2, _, iters2, _, f2 = run_kernel(
        ext.fused_laplace_newton, c, dev, f0, TOL, 40)
    assert same_bits(f2, f) and same_bits(psi2, psi)
    assert same_bits(iters2, iters)
    logz2, grad2, *_ = run_kernel(
        ext.fused_laplace_evidence, c, dev, f0, TOL, 40)
    assert same_bits(logz2, logz)
    for e in range(c.E):
        grads_close(grad2[e], grad[e])

    for e in range(c.E):
        psi1, _, iters1, bad1, f1 = run_kernel(
            ext.fused_laplace_newton, c, dev, f0, TOL, 40, rows=[e])
        assert same_bits(f1[0], f[e]), e
        assert same_bits(psi1[0], psi[e]), e
        assert int(iters1[0]) == int(iters[e]), e
        logz1, grad1, *_ = run_kernel(
            ext.fused_laplace_evidence, c, dev, f0, TOL, 40, rows=[e])
        assert same_bits(logz1[0], logz[e]), e
        grads_close(grad1[0], grad[e])


# ---------------------------------------------------------------------------
# 5. the dispatcher below the tolerance floor
# ---------------------------------------------------------------------------

def test_dispatcher_below_tolerance_floor(dev, ext, monkeypatch):
    """tol = 1e-8 < LAPLACE_MIN_TOL: ``ops.laplace_nll_grad`` runs the fused
    Newton loop, then the torch polish; the fused evidence is not used."""
    from spark_gp_amd import ops
    from spark_gp_amd.ops import hip_backend, torch_backend
    E, k, d, tol = 6, 65, 7, 1e-8
    assert tol < hip_backend.LAPLACE_MIN_TOL
    c = make_inputs(E, k, d, "ard", 1.0, 1e-2, seed=55)
    calls = {"newton": 0, "evidence": 0}
    real_newton = hip_backend.laplace_newton
    real_evidence = hip_backend.laplace_evidence

    def counted_newton(*a, **kw):
        calls["newton"] += 1
        return real_newton(*a, **kw)

    def counted_evidence(*a, **kw):
        calls["evidence"] += 1
        return real_evidence(*a, **kw)

    monkeypatch.setattr(hip_backend, "laplace_newton", counted_newton)
    monkeypatch.setattr(hip_backend, "laplace_evidence", counted_evidence)
    f = torch.zeros(E, k, device=dev)
    nll, grad = ops.laplace_nll_grad(c.kern, c.theta, c.X.to(dev),
                                     c.y.to(dev), f, tol)
    assert calls == {"newton": 1, "evidence": 0}
    nll_ref, grad_ref = torch_backend.laplace_nll_grad(
        c.kern, c.theta, c.X64, c.y64, torch.zeros(E, k, dtype=TD), tol)
    assert nll == pytest.approx(nll_ref, rel=1e-3)
    np.testing.assert_allclose(grad, grad_ref, rtol=2e-2,
                               atol=1e-3 * np.abs(grad_ref).max())
