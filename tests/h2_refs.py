"""Reference computations that more than one H2MC test file shares (tests/test_gpu_h2mc.py, tests/test_gpu_coop_lists.py): the golden bar of the step's Hessian
launch and the float64 numpy.linalg.eigh recomputation of the proposal Gaussian with its inputs.  Plain NumPy; what a test asserts with them is the test's."""
import numpy as np


def golden_hessian_errors(z, i, dim, loglum, grad, hess):
    """State i of tests/golden/derv_vectors_full.npz (z) against a device result (loglum, grad[dim], hess[dim, dim]): the reference programs' gradient and
    the triangle of the Hessian that Eigen reads (h2mc.cpp:78: the UPPER triangle of the rows as delivered).  Returns None where the reference itself is
    not finite, else (relative gradient error, relative Hessian error); asserts logLum within 5e-3."""
    H1 = z["h2_hess"][i][: dim * dim].reshape(dim, dim)
    G1 = z["h2_grad"][i][:dim]
    if not (np.isfinite(H1).all() and np.isfinite(G1).all()):
        return None
    assert abs(loglum - z["loglum"][i]) < 5e-3
    iu = np.triu_indices(dim)
    eg = np.linalg.norm(G1 - grad) / max(np.linalg.norm(G1), 1e-2)
    eh = np.linalg.norm(H1[iu] - hess[iu]) / max(np.linalg.norm(H1[iu]), 1e-1)
    return float(eg), float(eh)


def gauss_eigh_inputs(dim, n=512, sigma=0.01):
    """n symmetric Hessians of dimension dim (float64), gradients and offsets: every fourth matrix well conditioned, ill-conditioned (eigenvalues over five
    decades, mixed signs -- condition numbers up to 1e5: beyond ~1e6 single precision no longer separates the small eigenvalues' vectors, whatever the solver),
    rank deficient, below the early-out norm.  Deterministic in (dim, n)."""
    rng = np.random.default_rng(100 + dim)
    H = np.zeros((n, dim, dim))
    for i in range(n):
        Q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
        kind = i % 4
        if kind == 0:
            ev = rng.standard_normal(dim) * 10.0 ** rng.uniform(3, 6)
        elif kind == 1:  # ill-conditioned: eigenvalues spread over five decades, mixed signs
            ev = np.sign(rng.standard_normal(dim)) * 10.0 ** rng.uniform(1, 6, dim)
        elif kind == 2:  # rank deficient with EXACT zeros (a block of zero rows / columns: the |w| <= 1e-10 branch of h2mc.cpp:100-118; zeros that
            # only exist up to rounding would make the sign of those eigenvalues -- and with it the cosh / cos remap -- a coin toss on both sides)
            m = max(2, dim // 2)
            Qm, _ = np.linalg.qr(rng.standard_normal((m, m)))
            H[i, :m, :m] = (Qm * (rng.standard_normal(m) * 1e5)) @ Qm.T
            continue
        else:  # below the early-out norm (hnorm < 0.5 / sigma^2 = 5000)
            ev = rng.standard_normal(dim) * 100.0
        H[i] = (Q * ev) @ Q.T
    H = (H + H.transpose(0, 2, 1)) / 2
    grad = rng.standard_normal((n, dim)) * 10.0 ** rng.uniform(0, 3, (n, 1))
    offset = rng.standard_normal((n, dim)) * sigma
    return H, grad, offset


def check_gauss_against_eigh(out, px, H, grad, offset, sigma):
    """Device Gaussians out[n, 544] (mean 16 | logDet | kind | .. | covL at 32 | invCov at 288) and px[n] (None: not checked) of the float32 roundings of
    H[n, dim, dim], grad[n, dim], offset[n, dim] against a float64 recomputation of h2mc.cpp:3-142 with numpy.linalg.eigh: mean, invCov, covL covL^T, logDet
    -- the quantities that do not depend on the eigenvector convention -- and px = log N(-offset; mean, invCov^-1).  Asserts every state; returns
    (dense records, isotropic records)."""
    n, dim = H.shape[0], H.shape[1]
    inv_s2 = 1.0 / (sigma * sigma)
    H32, g32, o32 = H.astype(np.float32).astype(np.float64), grad.astype(np.float32).astype(np.float64), offset.astype(np.float32).astype(np.float64)
    L = np.pi / 2
    pos_s, pos_o = np.sinh(L) ** 2, 0.5 * (np.exp(L) + np.exp(-L) - 1.0)  # h2mc.h:10-16
    neg_s, neg_o = np.sin(L) ** 2, -(np.cos(L) - 1.0)
    n_dense = n_iso = 0
    for i in range(n):
        Hs = np.triu(H32[i]) + np.triu(H32[i], 1).T  # the triangle Eigen reads
        hnorm = np.sqrt((Hs ** 2).sum())
        kind = out[i, 17]
        if hnorm < 0.5 * inv_s2 * (1 - 1e-5):
            assert kind == 1.0, (i, hnorm)
        if kind == 1.0:  # isotropic early-out, h2mc.cpp:84-92
            n_iso += 1
            assert hnorm < 0.5 * inv_s2 * (1 + 1e-5)
            assert abs(out[i, 16] - dim * np.log(inv_s2)) < 1e-3 * dim
            ref_px = dim * (-0.9189385332046727) + 0.5 * dim * np.log(inv_s2) - 0.5 * inv_s2 * (o32[i] ** 2).sum()
            assert px is None or abs(px[i] - ref_px) < 1e-3 * max(1.0, abs(ref_px))
            continue
        n_dense += 1
        w, V = np.linalg.eigh(Hs)
        eb = np.where(np.abs(w) > 1e-10, 1.0 / np.maximum(np.abs(w), 1e-300), 0.0)
        ob = eb * (V.T @ g32[i])
        s2 = np.where(np.abs(w) > 1e-10, np.where(w > 0, pos_s, neg_s), L * L)
        oo = np.where(np.abs(w) > 1e-10, ob * np.where(w > 0, pos_o, neg_o), 0.5 * ob * L * L)
        e2 = eb * s2
        e2 = np.where(e2 > 1e-10, 1.0 / np.maximum(e2, 1e-300), 0.0)
        post = e2 + inv_s2
        mean = V @ ((e2 / post) * oo)
        inv_cov = (V * post) @ V.T
        cov = (V / post) @ V.T
        log_det = np.log(post).sum()
        d_mean, d_cl, d_ic = out[i, :dim].astype(np.float64), out[i, 32:32 + dim * dim].reshape(dim, dim).astype(np.float64), out[i, 288:288 + dim * dim].reshape(dim, dim).astype(np.float64)
        assert np.linalg.norm(d_ic - inv_cov) <= 2e-3 * np.linalg.norm(inv_cov), (i, kind)
        assert np.linalg.norm(d_cl @ d_cl.T - cov) <= 2e-3 * np.linalg.norm(cov), i
        assert np.linalg.norm(d_mean - mean) <= 5e-3 * max(np.linalg.norm(mean), sigma), (i, np.linalg.norm(d_mean - mean), np.linalg.norm(mean))
        assert abs(out[i, 16] - log_det) <= 2e-3 * dim, i
        if px is not None:
            dd = -o32[i] - mean
            ref_px = dim * (-0.9189385332046727) + 0.5 * log_det - 0.5 * dd @ inv_cov @ dd
            assert abs(px[i] - ref_px) <= 5e-3 * max(1.0, abs(ref_px)), (i, px[i], ref_px)
    return n_dense, n_iso
