"""Float64 restatements of the inference layer, written from the definitions in plain numpy and sharing nothing with
``gigalens_amd/inference.py``: the Adam step, the Gaussian surrogate of SVI (sample and fused ELBO buffer), the leapfrog pieces and
the Metropolis step of the preconditioned HMC, and the HMC loop with its adaptation off -- with what a float32 evaluation of each
may differ from float64 by.  Every function also runs in float32 (``dtype``), in the kernels' operation order, as the yardstick
of the multi-step gates and as the subject of the mutation checks (``mutate``: one plausible wrong variant each).

Error bounds.  Higham's gamma_n = n u / (1 - n u), u = 2^-24, times the sum of the |terms| of an element (Accuracy and Stability
of Numerical Algorithms, section 3.1; like ``post_cases.gamma`` and ``point_image_cases.render_bound``).  n is read off the
summation structure of the kernel in ``csrc/gl_updates.hip.h`` and stated per function; ``expf`` / ``logf`` count 4 u (2 ulp),
``sqrtf`` and a division one rounding.  A fused multiply-add only removes roundings.  Nothing in a bound is measured on a kernel.
Results below the smallest normal float32 may be flushed: every bound carries ``TINY`` = 2^-126 as an absolute floor."""
import math

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
LOG_2PI = math.log(2.0 * math.pi)
HYPER = dict(lr=3e-2, b1=0.9, b2=0.999, eps=1e-7, scale=1.0)


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def f32(x):
    """the float32 nearest to a host double: what a ``float`` argument of a C entry point receives"""
    return float(np.float32(x))


def _as(T, *arrays):
    return tuple(np.asarray(a).astype(T) for a in arrays)


# ---- Adam -------------------------------------------------------------------------------------------------------------------
def adam64(x, m, v, grad, hyper, t, dtype=np.float64, mutate=None):
    """One textbook Adam step at count ``t`` (the count of THIS step, from 1): returns ``(x', m', v')``.  The hyper-parameters
    are taken at their float32 values (the C entry takes floats: the kernel is Adam at float32(0.999)); the bias corrections
    1 - beta^t are formed in double from those, and in float32 mode rounded to float32 like the kernel's arguments.  1 - beta is
    exact in float32 for beta in [0.5, 1].  ``mutate='no_c2'``: the second bias correction dropped."""
    T = dtype
    h = {k: f32(hyper[k]) for k in ("lr", "b1", "b2", "eps", "scale")}
    c1, c2 = 1.0 - h["b1"] ** float(t), 1.0 - h["b2"] ** float(t)
    if mutate == "no_c2":
        c2 = 1.0
    lr, b1, b2, eps, s, c1, c2, one = (T(a) for a in (h["lr"], h["b1"], h["b2"], h["eps"], h["scale"], c1, c2, 1.0))
    x, m, v, g = _as(T, x, m, v, grad)
    with np.errstate(all="ignore"):
        g = g * s
        mi = m * b1 + g * (one - b1)
        vi = v * b2 + (g * g) * (one - b2)
        xn = x - lr * (mi / c1) / (np.sqrt(vi / c2) + eps)
    return xn, mi, vi


def adam_bound(x, m, v, grad, hyper, t):
    """``(bx, bm, bv)`` for one step from a given float32 state.  m': the rounding of g = grad * scale, a product and the addition
    on each term: gamma_3 (|m b1| + |g (1 - b1)|).  v': g twice, g g, the product with 1 - b2, the addition: gamma_5 v' (all
    terms positive).  The update lr (m'/c1) / (sqrt(v'/c2) + eps): the error of m' carried through, and on the rest 9.5 roundings
    -- c2, the division, half of those 7 through the square root, the square root, the addition of eps (5.5); c1, its division,
    the product with lr, the last division (4) -- taken as gamma_10; then half an ulp of x'."""
    h = {k: f32(hyper[k]) for k in ("lr", "b1", "b2", "eps", "scale")}
    xn, mi, vi = adam64(x, m, v, grad, hyper, t)
    g = np.asarray(grad, dtype=np.float64) * h["scale"]
    bm = gamma(3) * (np.abs(np.asarray(m, dtype=np.float64) * h["b1"]) + np.abs(g * (1.0 - h["b1"]))) + TINY
    bv = gamma(5) * vi + TINY
    c1, c2 = 1.0 - h["b1"] ** float(t), 1.0 - h["b2"] ** float(t)
    den = np.sqrt(vi / c2) + h["eps"]
    upd = np.abs(h["lr"] * (mi / c1) / den)
    bu = h["lr"] / (c1 * den) * bm * (1.0 + gamma(10)) + gamma(10) * upd
    bx = bu + U * (np.abs(xn) + bu) + TINY
    return bx, bm, bv


# ---- the packed lower triangle ----------------------------------------------------------------------------------------------
def tril_rows(d):
    """(j, k) of packed index t, row-major over the lower triangle: t = j (j + 1) / 2 + k, k <= j"""
    return np.tril_indices(d)


def tril_jk32(t, mutate=None):
    """The kernel's way from t to (j, k): a float32 square-root seed and two fix-up loops.  ``mutate='row_start'``: the second
    loop steps back at equality too, so the first element of a row lands one row up (j - 1, k = j)."""
    j = int((np.sqrt(np.float32(8.0) * np.float32(t) + np.float32(1.0)) - np.float32(1.0)) * np.float32(0.5))
    while (j + 1) * (j + 2) // 2 <= t:
        j += 1
    while (j * (j + 1) // 2 >= t and t > 0) if mutate == "row_start" else (j * (j + 1) // 2 > t):
        j -= 1
    return j, t - j * (j + 1) // 2


# ---- the Gaussian surrogate -------------------------------------------------------------------------------------------------
def _scale_tril(lp, d, full_rank, shift, T):
    """L of the surrogate and e = exp(p_jj): FillScaleTriL(Exp, diag_shift) over the row-major packing, or diag(exp(p))"""
    L = np.zeros((d, d), dtype=T)
    if full_rank:
        L[tril_rows(d)] = lp
        e = np.exp(np.diagonal(L).copy())
        L[np.arange(d), np.arange(d)] = e + T(shift)
    else:
        e = np.exp(lp)
        L[np.arange(d), np.arange(d)] = e
    return L, e


def svi_sample64(mu, lp, eps, full_rank, diag_shift, dtype=np.float64):
    """z_i = mu + L eps_i, ``(n, d)``.  Mean field: L = diag(exp(p)), the shift is not applied (at d = 1 the two surrogates are
    mu + (exp(p) + shift) eps and mu + exp(p) eps)."""
    T = dtype
    mu, lp, eps = _as(T, mu, lp, eps)
    L, _ = _scale_tril(lp, mu.size, full_rank, f32(diag_shift), T)
    return mu[None, :] + np.einsum("jk,ik->ij", L, eps)


def svi_sample_bound(mu, lp, eps, full_rank, diag_shift):
    """Element (i, j): mu_j and the j + 1 products of row j added one after the other -- j + 1 additions, one rounding per
    product, one for exp(p) + shift: gamma_{j+3} (|mu_j| + sum_k |L_jk eps_ik|) -- plus 4 u |exp(p_jj) eps_ij| for ``expf``.
    Mean field is row 0's count for every j."""
    mu, lp, eps = _as(np.float64, mu, lp, eps)
    d = mu.size
    L, e = _scale_tril(lp, d, full_rank, f32(diag_shift), np.float64)
    terms = np.abs(mu)[None, :] + np.abs(eps) @ np.abs(L).T
    n = (np.arange(d) if full_rank else np.zeros(d)) + 3
    return gamma(n)[None, :] * terms + 4.0 * U * np.abs(eps) * e[None, :] + TINY


def svi_buffer64(lp, eps, logp, G, full_rank, diag_shift, dtype=np.float64, mutate=None):
    """The fused buffer ``[ELBO, dELBO/dmu (d), dELBO/dp (packed)]`` from given draws, log-densities and gradients G = dlogp/dz:
    ELBO = mean(log q - log p), log q = -1/2 |eps|^2 - log det L - d/2 log 2 pi;  d/dmu_j = -mean G_j;  d/dL_jk = -mean G_j eps_k
    on the lower triangle;  on the diagonal L_jj = exp(p_jj) + shift gives d/dp_jj = v e - e / (e + shift) (the second term from
    -log det L), mean field v e - 1, with v = d/dL_jj and e = exp(p_jj).  ``mutate='no_shift'``: the shift left out of that
    derivative;  ``mutate='row_start'``: packed outputs placed through the mutated :func:`tril_jk32`."""
    T = dtype
    lp, eps, logp, G = _as(T, lp, eps, logp, G)
    n, d = eps.shape
    shift = T(f32(diag_shift))
    L, e = _scale_tril(lp, d, full_rank, shift, T)
    q = np.einsum("ik,ik->i", eps, eps)
    log_det = np.log(np.diagonal(L)).sum() if full_rank else lp.sum()
    elbo = (T(-0.5) * q - logp).sum() / T(n) - log_det - T(0.5 * d) * T(f32(LOG_2PI) if T is np.float32 else LOG_2PI)
    g_mu = -G.sum(0) / T(n)
    if full_rank:
        M = -np.einsum("ij,ik->jk", G, eps) / T(n)
        if mutate == "row_start":
            jk = np.array([tril_jk32(t, mutate) for t in range(d * (d + 1) // 2)])
            jj, kk = jk[:, 0], jk[:, 1]
        else:
            jj, kk = tril_rows(d)
        g_p = M[jj, kk]
        on = jj == kk
        ratio = T(1.0) if mutate == "no_shift" else e[jj[on]] / (e[jj[on]] + shift)
        g_p[on] = g_p[on] * e[jj[on]] - ratio
    else:
        g_p = -np.einsum("ij,ij->j", G, eps) / T(n) * e - T(1.0)
    return np.concatenate([np.reshape(elbo, 1), g_mu, g_p]).astype(T)


def svi_reduction_roundings(n):
    """One output of gl_svi_grad_kernel: ceil(n / 256) additions per thread, 6 DPP additions across the wave, 3 across the four
    waves, the division by n, and the product (or the -1/2 q - logp) that forms an addend."""
    return -(-n // 256) + 6 + 3 + 1 + 1


def svi_buffer_bound(lp, eps, logp, G, full_rank, diag_shift):
    """Per output, with r = :func:`svi_reduction_roundings`.  d/dmu_j: gamma_r mean |G_j|;  d/dL_jk: gamma_r mean |G_j eps_k|.
    Diagonal: e times that, gamma_6 |v e| (expf 4 u, the product, the subtraction) and gamma_11 e / (e + shift) (expf in the
    numerator and in the denominator, the addition, the division, the subtraction); mean field e times that, gamma_5 |v e| and
    half an ulp of the result v e - 1.  ELBO: the d-term
    inner sum, the -1/2 q - logp and the reduction, gamma_{d+2+r} mean(1/2 q + |logp|);  log det L = sum of d terms
    logf(expf(p) + shift), each 5 u absolute (expf and the addition, through the logarithm) + 4 u |term|, then d additions and the
    three that join it, d/2 log 2 pi and the mean: gamma_{d+3} (sum |terms| + d/2 log 2 pi + |mean|)."""
    lp, eps, logp, G = _as(np.float64, lp, eps, logp, G)
    n, d = eps.shape
    r = svi_reduction_roundings(n)
    shift = f32(diag_shift)
    L, e = _scale_tril(lp, d, full_rank, shift, np.float64)
    q = (eps * eps).sum(1)
    mean0 = (0.5 * q + np.abs(logp)).mean()
    ld = np.abs(np.log(np.diagonal(L))) if full_rank else np.abs(lp)
    b_elbo = gamma(d + 2 + r) * mean0 + (float((5.0 * U + 4.0 * U * ld).sum()) if full_rank else 0.0) \
        + gamma(d + 3) * (ld.sum() + 0.5 * d * LOG_2PI + mean0)
    b_mu = gamma(r) * np.abs(G).mean(0) + TINY
    A = np.abs(G).T @ np.abs(eps) / n
    if full_rank:
        jj, kk = tril_rows(d)
        b_p = gamma(r) * A[jj, kk] + TINY
        on = jj == kk
        v = (-(G.T @ eps) / n)[jj[on], kk[on]]
        b_p[on] = e * b_p[on] + gamma(6) * np.abs(v * e) + gamma(11) * e / (e + shift)
    else:
        v = -(G * eps).mean(0)
        b_p = e * (gamma(r) * np.diagonal(A) + TINY) + gamma(5) * np.abs(v * e) + U * np.abs(v * e - 1.0)
    return np.concatenate([[b_elbo], b_mu, b_p])


# ---- the leapfrog pieces ----------------------------------------------------------------------------------------------------
def kick_drift64(p, g, kick, z, sigma, eps, dtype=np.float64, mutate=None):
    """p' = p + kick g,  z' = z + eps p' Sigma.  ``kick`` and ``eps`` at their float32 values.  ``mutate='kick_sign'``."""
    T = dtype
    p, g, z, sigma = _as(T, p, g, z, sigma)
    k = T(f32(kick)) * (T(-1.0) if mutate == "kick_sign" else T(1.0))
    pn = p + k * g
    return pn, z + T(f32(eps)) * (pn @ sigma)


def kick_drift_bound(p, g, kick, z, sigma, eps):
    """``(bp, bz)``.  p': a product and an addition, gamma_2 (|p| + |kick g|).  z'_j: the d terms p'_k Sigma_kj added one after the
    other, the product with eps and the addition of z: gamma_{d+3} (|eps| sum_k |p'_k Sigma_kj| + |z_j|); the sum runs over the
    ROUNDED p', which adds |eps| sum_k bp_k |Sigma_kj|."""
    p, g, z, sigma = _as(np.float64, p, g, z, sigma)
    d = p.shape[1]
    bp = gamma(2) * (np.abs(p) + np.abs(f32(kick) * g)) + TINY
    pn = p + f32(kick) * g
    bz = abs(f32(eps)) * (bp @ np.abs(sigma)) + gamma(d + 3) * (abs(f32(eps)) * (np.abs(pn) @ np.abs(sigma)) + np.abs(z)) + TINY
    return bp, bz


def _pL(p, L, mutate):
    return p @ (L if mutate == "upper" else np.tril(L))


def accept64(z, g, lp, zn, gn, lpn, p0, pn, kick, L, u, dtype=np.float64, mutate=None):
    """The close of a transition: last half kick p1 = pn + kick gn, kinetic energies ke = 1/2 |p L|^2 with L lower triangular
    (what lies above the diagonal is never read), log_acc = (lpn - ke1) - (lp - ke0), a non-finite log_acc is a rejection
    (-inf), acceptance probability exp(min(log_acc, 0)), decision log u < log_acc, state selected per chain.
    ``mutate='upper'``: the whole matrix read;  ``mutate='no_last_kick'``."""
    T = dtype
    z, g, lp, zn, gn, lpn, p0, pn, L, u = _as(T, z, g, lp, zn, gn, lpn, p0, pn, L, u)
    with np.errstate(all="ignore"):
        p1 = pn if mutate == "no_last_kick" else pn + T(f32(kick)) * gn
        s0, s1 = _pL(p0, L, mutate), _pL(p1, L, mutate)
        ke0, ke1 = T(0.5) * (s0 * s0).sum(-1), T(0.5) * (s1 * s1).sum(-1)
        raw = (lpn - ke1) - (lp - ke0)
        log_acc = np.where(np.isfinite(raw), raw, -np.inf).astype(T)
        log_u = np.log(u)
        take = log_u < log_acc
        acc_prob = np.exp(np.minimum(log_acc, T(0.0)))
        margin = np.abs(log_u.astype(np.float64) - log_acc.astype(np.float64))
        margin = np.where(np.isnan(margin), np.inf, margin)  # log u = log_acc = -inf: a rejection either way
    sel = take[:, None]
    return dict(log_acc=log_acc, acc_prob=acc_prob, take=take, margin=margin, ke0=ke0, ke1=ke1,
                z=np.where(sel, zn, z), g=np.where(sel, gn, g), lp=np.where(take, lpn, lp))


def accept_bound(lp, gn, lpn, p0, pn, kick, L, u):
    """``(b_log_acc, b_acc_prob, b_decision)`` per chain.  Column k of p L: the d - k terms p_j L_jk added one after the other,
    bs_k = gamma_{d-k+1} sum_j |p_j L_jk| (+ sum_j bp1_j |L_jk| for the kicked momentum, bp1 = gamma_2 (|pn| + |kick gn|)); its
    square 2 |s_k| bs_k + bs_k^2 and one rounding; the squares summed over ceil(d / 128) additions per thread, 6 DPP additions and
    one across the two waves: gamma_{ceil(d/128)+8} sum s_k^2.  log_acc joins four terms with three subtractions: gamma_3 of their
    magnitudes.  acc_prob: exp(min(., 0)) over the interval log_acc +- b, and 4 u for ``expf``.  The decision compares with
    ``logf(u)``, 4 u |log u| more."""
    lp, gn, lpn, p0, pn, L, u = _as(np.float64, lp, gn, lpn, p0, pn, L, u)
    d = p0.shape[1]
    Lt = np.tril(L)
    gcol = gamma(d - np.arange(d) + 1)[None, :]
    r = gamma(-(-d // 128) + 8)
    with np.errstate(all="ignore"):
        p1 = pn + f32(kick) * gn
        bp1 = gamma(2) * (np.abs(pn) + np.abs(f32(kick) * gn)) + TINY

        def ke_bound(p, bp):
            s = p @ Lt
            bs = gcol * (np.abs(p) @ np.abs(Lt)) + (0.0 if bp is None else bp @ np.abs(Lt))
            return 0.5 * (s * s).sum(-1), 0.5 * ((2.0 * np.abs(s) * bs + bs * bs).sum(-1) + r * (s * s).sum(-1))

        ke0, b0 = ke_bound(p0, None)
        ke1, b1 = ke_bound(p1, bp1)
        raw = (lpn - ke1) - (lp - ke0)
        ok = np.isfinite(raw)
        b_la = np.where(ok, b0 + b1 + gamma(3) * (np.abs(lpn) + ke1 + np.abs(lp) + ke0), 0.0)
        la = np.where(ok, raw, -np.inf)
        a = np.exp(np.minimum(la, 0.0))
        hi, lo = np.exp(np.minimum(la + b_la, 0.0)), np.exp(np.minimum(la - b_la, 0.0))
        b_acc = np.where(ok, np.maximum(hi - a, a - lo), 0.0) + 4.0 * U * a + TINY
        log_u = np.abs(np.log(u))
        b_dec = b_la + np.where(np.isfinite(log_u), 4.0 * U * log_u, 0.0)
    return b_la, b_acc, b_dec


# ---- the HMC loop with its adaptation off -----------------------------------------------------------------------------------
def halton2(i):
    f, r = 0.5, 0.0
    while i > 0:
        r, i, f = r + f * (i & 1), i >> 1, 0.5 * f
    return r


def hmc_transitions64(vg64, mean, L, eps, init_l, n, K, max_leapfrog, draws, dtype=np.float64, mutate=None):
    """``ModellingSequence.HMC`` with ``num_burnin_steps = 0`` restated: chains start at mean + L xi; momentum p = L^-T xi (mass
    = the inverse of Sigma = L L^T); the trajectory length T = eps * init_l is fixed and transition ``it`` takes
    ceil(halton2(it + 1) T / eps) leapfrog steps within [1, max_leapfrog]: half kick, then drift / kick ..., the last kick a half
    one; Metropolis test with the kinetic energy 1/2 |p L|^2; a non-finite log_acc is a rejection.  ``draws`` is consumed in the
    loop's order: randn(n, d) for the start, then per transition randn(n, d) for the momenta and rand(n) for the test.
    ``vg64(z) -> (log p, d log p / dz)`` in the dtype it is given.  Returns the states after every transition ``(K, n, d)``, the
    margins |log u - log_acc| ``(K, n)`` and ``dict(log_acc, take)``.  ``mutate``: 'no_last_kick', 'kick_sign'."""
    T = dtype
    draws = iter(draws)
    L32 = np.asarray(L, dtype=np.float32)
    Linv_T = np.linalg.inv(L32.astype(np.float64)).T.astype(T)  # the loop inverts in double and hands the kernels float32
    Lt, mean = L32.astype(T), np.asarray(mean, dtype=np.float32).astype(T)
    sigma = Lt @ Lt.T
    step = math.exp(math.log(eps))
    length = eps * min(max(int(init_l), 1), max_leapfrog)
    e, h = T(f32(step)), T(f32(0.5 * step))
    sign = T(-1.0) if mutate == "kick_sign" else T(1.0)
    z = mean[None, :] + np.asarray(next(draws)).astype(T) @ Lt.T
    assert z.shape[0] == n
    lp, g = vg64(z)
    states, margins, las, takes = [], [], [], []
    for it in range(K):
        n_leap = int(min(max(math.ceil(halton2(it + 1) * length / step), 1), max_leapfrog))
        xi, u = np.asarray(next(draws)).astype(T), np.asarray(next(draws)).astype(T)
        p0 = xi @ Linv_T.T
        pn, zn = p0 + sign * h * g, z
        for i in range(n_leap):
            zn = zn + e * (pn @ sigma)
            lpn, gn = vg64(zn)
            if i < n_leap - 1:
                pn = pn + sign * e * gn
        a = accept64(z, g, lp, zn, gn, lpn, p0, pn, float(sign) * float(h), Lt, u, dtype=T,
                     mutate="no_last_kick" if mutate == "no_last_kick" else None)
        z, g, lp = a["z"], a["g"], a["lp"]
        states.append(z)
        margins.append(a["margin"])
        las.append(a["log_acc"].astype(np.float64))
        takes.append(a["take"])
    return np.stack(states), np.stack(margins), dict(log_acc=np.stack(las), take=np.stack(takes))


def transitions_gate(got, r64, r32):
    """The gate of a loop's states ``got (K, n, d)`` against the float64 restatement on the same draws, from the float32 run of
    the restatement alone.  yard_la: the worst |log_acc32 - log_acc64| over the chains whose float32 decisions agreed with float64
    up to the transition before; yard_z: the worst |z32 - z64| over the chains that agree through the transition, as a fraction of
    max |z64|.  A chain is left out from the first transition where its float64 margin is below 4 yard_la.  Returns ``dict(err,
    yard_z, yard_la, left_out, flipped32)``: the gate is err <= 4 yard_z and left_out <= 1 %."""
    z64, m64, i64 = r64
    z32, _, i32 = r32
    same = np.cumprod(i64["take"] == i32["take"], axis=0).astype(bool)            # agree through transition k
    before = np.concatenate([np.ones_like(same[:1]), same[:-1]], axis=0)           # ... up to the transition before
    dla = np.abs(i32["log_acc"] - i64["log_acc"])
    dla = np.where(np.isfinite(dla), dla, 0.0)                                      # both -inf: no deviation
    yard_la = float(dla[before].max())
    scale = float(np.abs(z64).max())
    yard_z = float(np.abs(z32.astype(np.float64) - z64).max(-1)[same].max()) / scale
    keep = np.cumprod(m64 >= 4.0 * yard_la, axis=0).astype(bool)
    err = float(np.abs(np.asarray(got, dtype=np.float64) - z64).max(-1)[keep].max()) / scale
    return dict(err=err, yard_z=yard_z, yard_la=yard_la, left_out=1.0 - float(keep[-1].mean()), flipped32=int((~same[-1]).sum()))


# ---- the known target of the loop tests -------------------------------------------------------------------------------------
def gaussian_target(d, seed=0):
    """``(m, C)``: C = A A^T / d + diag(0.25, 1, 4, 0.5, 2, ...), a correlated covariance with a spread of scales"""
    r = np.random.default_rng(1000 + seed)
    A = r.standard_normal((d, d))
    C = A @ A.T / d + np.diag(np.resize([0.25, 1.0, 4.0, 0.5, 2.0], d))
    return r.standard_normal(d), C


class GaussModel:
    """N(m, C), unnormalised (log p = -1/2 (z - m)^T C^-1 (z - m)), behind the ForwardProbModel surface the loops use"""
    include_pixels, include_positions, n_position = True, False, 0.0

    def __init__(self, m, C, device="cpu"):
        self.device = torch.device(device)
        self.m64, self.C64 = np.asarray(m, dtype=np.float64), np.asarray(C, dtype=np.float64)
        self.P64 = np.linalg.inv(self.C64)
        self.m = torch.as_tensor(self.m64, dtype=torch.float32).to(self.device)
        self.P = torch.as_tensor(self.P64, dtype=torch.float32).to(self.device)

    def init_centroids(self, bs):
        return None

    def log_prob_and_grad(self, simulator, z):
        r = z - self.m
        g = -(r @ self.P)
        return 0.5 * (r * g).sum(-1), torch.zeros(z.shape[0], device=z.device), g

    def vg(self, dtype):
        """the same density on numpy arrays of ``dtype``, for :func:`hmc_transitions64`"""
        m, P = self.m64.astype(np.float32).astype(dtype), self.P64.astype(np.float32).astype(dtype)

        def f(z):
            r = z - m
            g = -(r @ P)
            return dtype(0.5) * (r * g).sum(-1), g
        return f

    @property
    def log_Z(self):
        return 0.5 * len(self.m64) * LOG_2PI + 0.5 * np.linalg.slogdet(self.C64)[1]


def moment_z_scores(x, m, C):
    """Worst |z-score| of the coordinate means (standard error sigma_j / sqrt(n)) and of the covariance entries (standard error
    sqrt((C_jk^2 + C_jj C_kk) / (n - 1))) of n independent draws ``x (n, d)`` from N(m, C)"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    sd = np.sqrt(np.diagonal(C))
    z_mean = np.abs(x.mean(0) - m) / (sd / math.sqrt(n))
    S = np.cov(x.T, ddof=1).reshape(len(m), len(m))
    z_cov = np.abs(S - C) / np.sqrt((C * C + np.outer(np.diagonal(C), np.diagonal(C))) / (n - 1))
    return float(z_mean.max()), float(z_cov.max())


# ---- inputs -----------------------------------------------------------------------------------------------------------------
SMALL_P = float(np.log(np.float32(1e-6)))  # a diagonal parameter at which exp(p) equals the default diag_shift


def adam_case(n, seed=0):
    """a float32 state (x, m, v >= 0) and a gradient spanning 1e-3 .. 1e3"""
    r = np.random.default_rng(seed)
    x, m = r.standard_normal(n), 0.1 * r.standard_normal(n)
    v = r.uniform(0.0, 1.0, n) ** 2
    grad = r.standard_normal(n) * 10.0 ** r.uniform(-3.0, 3.0, n)
    return tuple(a.astype(np.float32) for a in (x, m, v, grad))


def svi_case(n, d, full_rank, seed=0):
    """(mu, lp, eps, logp, G): every third diagonal parameter at log(1e-6), log p of magnitude 1e5 (a 256 x 256 likelihood), G over
    five decades"""
    r = np.random.default_rng(seed)
    mu = 0.3 * r.standard_normal(d)
    pd = np.log(r.uniform(0.05, 0.25, d))
    pd[::3] = SMALL_P
    if full_rank:
        M = 0.05 * r.standard_normal((d, d))
        M[np.arange(d), np.arange(d)] = pd
        lp = M[tril_rows(d)]
    else:
        lp = pd
    eps = r.standard_normal((n, d))
    logp = -1e5 * (1.0 + 0.1 * r.standard_normal(n))
    G = r.standard_normal((n, d)) * 10.0 ** r.uniform(-2.0, 3.0, (n, d))
    return tuple(a.astype(np.float32) for a in (mu, lp, eps, logp, G))


def index_map_case(d=300):
    """n = 1, G_j = j + 1, eps_k = (k + 1) / 1024: the off-diagonal output (j, k) is -(j + 1)(k + 1) / 1024 exactly in float32
    ((j + 1)(k + 1) < 2^24, one addend, division by 1).  Returns (lp, eps, logp, G, jj, kk, exact)."""
    jj, kk = tril_rows(d)
    lp = np.where(jj == kk, -1.0, 0.0).astype(np.float32)
    eps = ((np.arange(d) + 1) / 1024.0).astype(np.float32)[None, :]
    G = (np.arange(d) + 1).astype(np.float32)[None, :]
    exact = (-(jj + 1.0) * (kk + 1.0) / 1024.0).astype(np.float32)
    assert np.array_equal(exact.astype(np.float64), -(jj + 1.0) * (kk + 1.0) / 1024.0)
    return lp, eps, np.zeros(1, dtype=np.float32), G, jj, kk, exact


def kick_case(n, d, seed=0):
    """(p, g, kick, z, Sigma, eps) with a dense symmetric Sigma"""
    r = np.random.default_rng(seed)
    A = r.standard_normal((d, d)) / math.sqrt(d)
    sigma = 0.5 * (A + A.T) + np.diag(r.uniform(0.3, 1.3, d))
    p, g, z = (r.standard_normal((n, d)).astype(np.float32) for _ in range(3))
    return p, g, 0.035, z, sigma.astype(np.float32), 0.07


def accept_case(n, d, seed=0):
    """dict of the inputs of the Metropolis step.  log_acc is spread like N(0, 2^2); every uniform is DESIGNED: log u sits at
    (2 + Exp(1)) x the derived bound on log_acc, plus for every other chain Exp(1) x 1e-3, from log_acc, on a random side where
    (0, 1) has room for it -- the closest decisions the bound still calls.  The caller asserts that float64 alone keeps
    at least 98 % of the chains."""
    r = np.random.default_rng(seed)
    L = np.tril(r.standard_normal((d, d))) * (0.5 / math.sqrt(d))
    L[np.arange(d), np.arange(d)] = r.uniform(0.3, 1.3, d)
    L = (L / math.sqrt(max(d / 16.0, 1.0))).astype(np.float32)
    z, g, zn, gn, p0, pn = (r.standard_normal((n, d)).astype(np.float32) for _ in range(6))
    lp = r.standard_normal(n).astype(np.float32)
    kick = 0.035
    p1 = pn.astype(np.float64) + f32(kick) * gn
    ke = lambda p: 0.5 * ((p.astype(np.float64) @ np.tril(L).astype(np.float64)) ** 2).sum(-1)
    lpn = (lp + ke(p1) - ke(p0) + 2.0 * r.standard_normal(n)).astype(np.float32)
    b_la, _, _ = accept_bound(lp, gn, lpn, p0, pn, kick, L, np.full(n, 0.5))
    la = (lpn.astype(np.float64) - ke(p1)) - (lp.astype(np.float64) - ke(p0))
    m = b_la * (2.0 + r.exponential(1.0, n)) + 1e-3 * r.exponential(1.0, n) * (np.arange(n) % 2)
    side = np.where(r.uniform(size=n) < 0.5, 1.0, -1.0)      # +1: log u below log_acc (accept)
    side = np.where(la + m > -1e-3, 1.0, side)               # no room above: below it is
    log_u = np.clip(la - side * m, -80.0, -1e-3)             # (an accept whatever u is keeps its margin when clipped)
    u = np.exp(log_u).astype(np.float32)
    assert (u > 0).all() and (u < 1).all()
    return dict(z=z, g=g, lp=lp, zn=zn, gn=gn, lpn=lpn, p0=p0, pn=pn, kick=kick, L=L, u=u)
