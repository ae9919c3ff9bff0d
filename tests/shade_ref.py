"""An independent restatement, in numpy, of the texture look-up and the three BSDFs the device evaluates (langevin-mcmc_amd/csrc/device/dshade.h, dmath.h):
Lambertian, Phong and the rough dielectric -- their Evaluate and Sample functions, the dielectric Fresnel term, Beckmann's D and G1, the micro-normal
sampler, the tangent frame, Reflect / Refract and the periodic bilinear bitmap look-up with its `fastpow` gamma (which is part of the operation's
definition).  Written from the formulas, vectorised over cases with masks, not line by line from the device source; where formula and device source
seemed to differ the reference implementation's lambertian.cpp, phong.cpp, roughdielectric.cpp, microfacet.h and bitmaptexture.h settled it (none
did in the end: see DESIGN.md "Shading probe").

dtype-generic: run(..., dtype=np.float64) is the reference; run(..., dtype=np.float32) is the same code in single precision, and the deviation of the
two over a family of cases is what a float implementation of these formulas may differ from the reference by (BARS below).

Besides the outputs every function reports its DECISIONS: every quantity the float code compares with a threshold, with the lanes that reach the
comparison.  `decisive(result)` says for which cases the reference is safely on one side of every threshold it reached:
  'abs'        cosines, sign products, uDiscrete - F, cosThetaT^2: dot products of unit vectors, a few float epsilons of error -> more than 1e-3 away
  'mag'        the magnitude thresholds 1e-10 / 1e-20 on exponent-dominated values (O(1) relative error) -> a factor of 10 away
  'underflow'  values a float evaluation may flush to zero: exactly 0, above 1e-30 or below 1e-50
  'exact'      comparisons of input words with constants or with each other (uDiscrete > KsWeight, n.z < -1 + 1e-6): the same in any precision
"""
import numpy as np

LAMBERTIAN, PHONG, ROUGHDIELECTRIC = 0, 1, 2
OP_TEX, OP_EVALUATE, OP_SAMPLE = 0, 1, 2
# a case's input row and output row (include/lmc_abi.h lmc_shade_probe)
IN_WI, IN_N, IN_WO, IN_ST, IN_RND, IN_U, IN_PDF, IN_REV, IN_COS, IN_CON = slice(0, 3), slice(3, 6), slice(6, 9), slice(9, 11), slice(11, 13), 13, 14, 15, 16, slice(17, 20)
OUT = dict(wo=slice(0, 3), contrib=slice(3, 6), cosWo=slice(6, 7), pdf=slice(7, 8), revPdf=slice(8, 9))

ABS_MARGIN = 1e-3
MAG_FACTOR = 10.0


class _K:
    """the float constants of the operation, in the working precision (each first rounded to float32: they are float literals in the definition)"""

    def __init__(self, T):
        self.T = T
        k = lambda x: T(np.float32(x))  # noqa: E731
        self.k = k
        self.eps = k(1e-4)
        self.pi = k(np.pi)
        self.nzflip = k(np.float32(-1.0 + 1e-6))


class Flow:
    """the lanes still alive in a function's control flow, and the record of every comparison they reached"""

    def __init__(self, n):
        self.alive = np.ones(n, bool)
        self.decisions = []  # (name, kind, q, threshold, reached, forced)

    def note(self, name, kind, q, thr, where=None, forced=None):
        reached = self.alive.copy() if where is None else (self.alive & where)
        self.decisions.append((name, kind, np.asarray(q, np.float64), float(thr), reached, forced))

    def leave(self, cond):
        gone = self.alive & cond
        self.alive = self.alive & ~cond
        return gone


def decisive(res, cos_margin=None):
    """[n] bool: the reference is decisively on one side of every threshold the case reached.  cos_margin (the conditioned set's construction): a
    wider margin for the cosines, and its square for the products of two"""
    ok = np.ones(len(res["ok"]), bool)
    for name, kind, q, thr, reached, forced in res["decisions"]:
        with np.errstate(all="ignore"):
            if kind == "abs":
                margin = ABS_MARGIN
                if cos_margin is not None and name.lstrip("|").startswith("cos") and "Theta" not in name:
                    margin = cos_margin**2 if "*" in name else cos_margin
                d = np.abs(q - thr) > margin
            elif kind == "mag":
                d = (q > thr * MAG_FACTOR) | (q < thr / MAG_FACTOR)
            elif kind == "underflow":
                a = np.abs(q)
                d = (a == 0) | (a > 1e-30) | (a < 1e-50)
            else:
                d = np.ones(len(q), bool)
        if forced is not None:
            d = d | forced
        ok &= d | ~reached
    return ok


# ------------------------------------------------------------------------------------------------ vectors
def dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def normalize(v):
    return v / np.sqrt(dot(v, v))[:, None]


def reflect(wi, n):
    """the mirror image of wi about n"""
    return (2 * dot(wi, n))[:, None] * n - wi


def refract(wi, n, cos_t, eta, inv_eta):
    """Snell: the transmitted direction for the signed cosine cos_t Fresnel returned (negative: wi arrives on n's side)"""
    e = np.where(cos_t < 0, inv_eta, eta)
    return n * (dot(wi, n) * e + cos_t)[:, None] - wi * e[:, None]


def coordinate_system(n, K):
    """the branch-free tangent frame around a unit vector (singular at -z, where a fixed frame takes over)"""
    flip = n[:, 2] < K.nzflip
    with np.errstate(all="ignore"):
        a = 1 / (1 + n[:, 2])
        b = -n[:, 0] * n[:, 1] * a
        one, zero = np.ones_like(a), np.zeros_like(a)
        b1 = np.stack([1 - n[:, 0] ** 2 * a, b, -n[:, 0]], 1)
        b2 = np.stack([b, 1 - n[:, 1] ** 2 * a, -n[:, 1]], 1)
    b1[flip] = np.stack([zero, -one, zero], 1)[flip]
    b2[flip] = np.stack([-one, zero, zero], 1)[flip]
    return b1, b2, flip


def to_world(local, b0, b1, n):
    return local[:, 0:1] * b0 + local[:, 1:2] * b1 + local[:, 2:3] * n


# ------------------------------------------------------------------------------------------------ textures
def fastpow(x, p, K):
    """Mineiro's fastpow2(p * fastlog2(x)): defined on the float32 bit pattern of x, returns a float32 bit pattern"""
    k, T = K.k, K.T
    vi = np.ascontiguousarray(x, np.float32).view(np.uint32)
    mx = ((vi & np.uint32(0x007FFFFF)) | np.uint32(0x3F000000)).view(np.float32).astype(T)
    y = vi.astype(T) * k(1.1920928955078125e-7)
    lg = y - k(124.22551499) - k(1.498030302) * mx - k(1.72587999) / (k(0.3520887068) + mx)
    q = (p * lg).astype(T)
    offset = np.where(q < 0, T(1), T(0))
    clipp = np.where(q < -126, T(-126), q)
    w = np.trunc(clipp)
    z = clipp - w + offset
    val = k(float(1 << 23)) * (clipp + k(121.2740575) + k(27.7280233) / (k(4.84252568) - z) - k(1.49012907) * z)
    return val.astype(np.int64).astype(np.uint32).view(np.float32).astype(T)


class Textures:
    """the caller's bitmap list: wh [nb, 2], gamma [nb], texels back to back"""

    def __init__(self, wh, gamma, texels):
        self.wh = np.asarray(wh, np.int64).reshape(-1, 2)
        self.gamma = np.asarray(gamma, np.float32)
        self.pool = np.asarray(texels, np.float32).ravel()
        self.off = np.concatenate([[0], np.cumsum(3 * self.wh[:, 0] * self.wh[:, 1])]).astype(np.int64)


def eval_tex(ref, st, tex, K):
    """ref: (bitmap [n] int, value [n, 3], sScale [n], tScale [n]).  A constant, or the bitmap's periodic bilinear value at (s sScale W - 1/2,
    t tScale H - 1/2) -- texel centres at half-integers, the texture wrapping in both directions -- clamped at 0 and raised to gamma by fastpow"""
    T = K.T
    bitmap, value, ss, ts = ref
    out = value.astype(T).copy()
    tx = bitmap >= 0
    if not tx.any():
        return out
    b = bitmap[tx]
    W, H = tex.wh[b, 0], tex.wh[b, 1]
    fs = ss[tx].astype(T) * st[tx, 0] * W.astype(T) - T(0.5)
    ft = ts[tx].astype(T) * st[tx, 1] * H.astype(T) - T(0.5)
    x0f, y0f = np.floor(fs), np.floor(ft)
    dx, dy = (fs - x0f)[:, None], (ft - y0f)[:, None]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    xa, xb, ya, yb = x0 % W, (x0 + 1) % W, y0 % H, (y0 + 1) % H

    def texel(x, y):
        return tex.pool[(tex.off[b] + (y * W + x) * 3)[:, None] + np.arange(3)[None, :]].astype(T)

    v = (1 - dx) * (1 - dy) * texel(xa, ya) + dx * (1 - dy) * texel(xb, ya) + (1 - dx) * dy * texel(xa, yb) + dx * dy * texel(xb, yb)
    v = np.maximum(v, T(0)).astype(T)
    out[tx] = fastpow(v, tex.gamma[b].astype(T)[:, None] * np.ones((1, 3), T), K)
    return out


# ------------------------------------------------------------------------------------------------ microfacets
def beckmann_d(h, alpha, K):
    """Beckmann's isotropic distribution of micro-normals, h in the frame of the surface normal: exp(-tan^2 / alpha^2) / (pi alpha^2 cos^4)"""
    c2 = h[:, 2] ** 2
    with np.errstate(all="ignore"):
        ex = (h[:, 0] ** 2 / alpha**2 + h[:, 1] ** 2 / alpha**2) / c2
        return np.exp(-ex) / (K.pi * alpha * alpha * c2**2)


def beckmann_g1(alpha, c, K, flow=None, name=None):
    """the rational approximation of Beckmann's shadowing term (Walter et al. 2007, eq. 27), 1 from a = 1 / (alpha tan) = 1.6 on"""
    k = K.k
    with np.errstate(all="ignore"):
        t = np.sqrt(np.abs(1 - c**2)) / c
        a = 1 / (alpha * t)
        g = (k(3.535) * a + k(2.181) * a * a) / (1 + k(2.276) * a + k(2.577) * a * a)
    if flow is not None:
        flow.note(name, "abs", np.where(t > 0, a, 1e9), 1.6, where=np.isfinite(a))
    return np.where((t <= 0) | (a >= k(1.6)), K.T(1), g)


def fresnel(cos_i, eta, inv_eta, K):
    """unpolarised Fresnel reflectance of a dielectric boundary for the signed cosine of incidence; also the signed cosine of the transmitted
    direction (0 and F = 1 under total internal reflection) and cos^2 of it, the quantity that decides"""
    T = K.T
    scale = np.where(cos_i > 0, inv_eta, eta)
    ct2 = 1 - (1 - cos_i**2) * scale**2
    tir = ct2 <= 0
    ci = np.abs(cos_i)
    with np.errstate(all="ignore"):
        ct = np.sqrt(np.where(tir, T(0), ct2))
        rs = (ci - eta * ct) / (ci + eta * ct)
        rp = (eta * ci - ct) / (eta * ci + ct)
    F = np.where(tir, T(1), T(0.5) * (rs**2 + rp**2))
    cos_t = np.where(tir, T(0), np.where(cos_i > 0, -ct, ct))
    return F.astype(T), cos_t.astype(T), ct2


def sample_micronormal(rnd, alpha, K):
    """a Beckmann micro-normal from two uniforms: tan^2 = -alpha^2 log(1 - u1), phi = 2 pi u2; 1 - u1 is clamped at 1e-6 inside the logarithm only"""
    k, T = K.k, K.T
    phi = 2 * K.pi * rnd[:, 1]
    tan2 = alpha**2 * (-np.log(np.maximum(1 - rnd[:, 0], k(1e-6))))
    c = 1 / np.sqrt(1 + tan2)
    pdf = (1 - rnd[:, 0]) / (K.pi * alpha**2 * c * c**2)
    s = np.sqrt(np.maximum(1 - c**2, T(0)))
    return np.stack([s * np.cos(phi), s * np.sin(phi), c], 1).astype(T), pdf.astype(T)


# ------------------------------------------------------------------------------------------------ the three BSDFs
class _Case:
    """a family's inputs in the working precision, the outputs initialised with what went in, and which words the operation wrote"""

    def __init__(self, mats, tex, ints, cin, T):
        self.K = K = _K(T)
        self.T, self.tex = T, tex
        self.n = n = len(cin)
        m = np.asarray(mats, np.float32)[ints[:, 0]]
        mi = m.view(np.int32)
        self.type, self.twoSided = mi[:, 0], mi[:, 1] != 0
        self.refs = {}
        for j, name in enumerate(("Kd", "Ks", "Kt", "expOrAlpha")):
            o = 2 + 6 * j
            self.refs[name] = (mi[:, o].astype(np.int64), m[:, o + 1 : o + 4], m[:, o + 4], m[:, o + 5])
        self.eta, self.invEta, self.KsWeight = m[:, 26].astype(T), m[:, 27].astype(T), m[:, 28].astype(T)
        self.adjoint = ints[:, 1] != 0
        c = np.asarray(cin)
        c = c if (c.dtype == np.float64 and T is np.float64) else c.astype(np.float32).astype(T)  # (float64 rows: the property tests' exact unit vectors)
        self.wi, self.nrm, self.wo0, self.st, self.rnd, self.u = c[:, IN_WI], c[:, IN_N], c[:, IN_WO], c[:, IN_ST], c[:, IN_RND], c[:, IN_U]
        self.out = dict(wo=c[:, IN_WO].copy(), contrib=c[:, IN_CON].copy(), cosWo=c[:, IN_COS].copy(), pdf=c[:, IN_PDF].copy(), revPdf=c[:, IN_REV].copy())
        self.written = {q: np.zeros(n, bool) for q in self.out}
        self.ok = np.ones(n, bool)
        self.flow = Flow(n)
        # a normal along an axis: its dot product with an input direction is one of that direction's words, exact in any precision
        self.axis = (np.sum(self.nrm == 0, 1) == 2) & (np.max(np.abs(self.nrm), 1) == 1)

    def texture(self, name):
        return eval_tex(self.refs[name], self.st, self.tex, self.K)

    def put(self, q, mask, value):
        value = np.asarray(value, self.T)
        if value.ndim < self.out[q].ndim:
            value = np.broadcast_to(value[..., None] if value.ndim else value, self.out[q].shape)
        else:
            value = np.broadcast_to(value, self.out[q].shape)
        self.out[q][mask] = value[mask]
        self.written[q] |= mask


def _facing(C):
    """the cosine of wi with the shading normal and the normal the function goes on with: a two-sided material turns the normal towards wi.
    Evaluate goes on with a negative cosine on a one-sided material (and finds it below the threshold); Sample gives up there."""
    cos_wi = dot(C.wi, C.nrm)
    turned = C.twoSided & (cos_wi < 0)
    n_ = np.where(turned[:, None], -C.nrm, C.nrm)
    return np.where(turned, -cos_wi, cos_wi), n_, cos_wi


def lambertian_evaluate(C, sel):
    K, T, f = C.K, C.T, C.flow
    f.alive = sel.copy()
    cos_wi, n_, _ = _facing(C)
    cos_wo = dot(n_, C.wo0)
    C.put("cosWo", sel, cos_wo)
    C.put("contrib", sel, T(0))
    f.note("cosWi", "abs", cos_wi, K.eps, forced=C.axis)
    f.leave(cos_wi < K.eps)
    f.note("cosWo", "abs", cos_wo, K.eps, forced=C.axis)
    f.leave(cos_wo < K.eps)
    a = f.alive
    C.put("contrib", a, (cos_wo / K.pi)[:, None] * C.texture("Kd"))
    C.put("pdf", a, cos_wo / K.pi)
    C.put("revPdf", a, cos_wi / K.pi)


def lambertian_sample(C, sel):
    K, T, f = C.K, C.T, C.flow
    f.alive = sel.copy()
    cos_wi, n_, raw = _facing(C)
    f.note("|cosWi|", "abs", np.abs(raw), K.eps, forced=C.axis)
    C.ok[f.leave(np.abs(raw) < K.eps)] = False
    C.ok[f.leave((raw < 0) & ~C.twoSided)] = False
    b0, b1, _ = coordinate_system(n_, K)
    f.note("n.z", "exact", n_[:, 2], K.nzflip)
    phi = 2 * K.pi * C.rnd[:, 0]
    r = np.sqrt(np.maximum(1 - C.rnd[:, 1], T(0)))
    z = np.sqrt(np.maximum(C.rnd[:, 1], T(0)))  # a cosine-weighted direction: the uniform disc sample lifted to the hemisphere
    a = f.alive.copy()
    C.put("wo", a, to_world(np.stack([np.cos(phi) * r, np.sin(phi) * r, z], 1), b0, b1, n_))
    C.put("cosWo", a, z)
    C.put("pdf", a, z / K.pi)
    f.note("cosWo", "abs", z, K.eps)
    C.ok[f.leave(z < K.eps)] = False
    a = f.alive
    C.put("revPdf", a, cos_wi / K.pi)
    C.put("contrib", a, C.texture("Kd"))


def _phong_lobes(C, f, live, cos_wi, cos_wo, R, wo, sample):
    """the normalised Phong lobe (n + 2) / (2 pi) cos^n around the mirror direction, picked with probability KsWeight and sampled with density
    (n + 1) / (2 pi) cos^n, plus the Lambertian lobe Kd / pi sampled by the cosine: (value before the cosine factor, pdf, reverse pdf, lobe taken)"""
    K, T, k = C.K, C.T, C.K.k
    kw = C.KsWeight
    expo = C.texture("expOrAlpha")[:, 0]
    spec, diff = kw > 0, kw < 1
    f.note("KsWeight>0", "exact", kw, 0, where=live)
    d = dot(R, wo)
    f.note("R.wo", "abs", d, 0, where=live & spec)
    with np.errstate(all="ignore"):
        weight = np.power(np.maximum(d, T(0)), expo) / (2 * K.pi)
    f.note("weight", "mag", weight, 1e-10, where=live & spec)
    lobe = spec & (weight > k(1e-10))
    contrib = np.where(lobe[:, None], C.texture("Ks") * ((expo + 2) * weight)[:, None], T(0))
    pdf = np.where(lobe, kw * (expo + 1) * weight, T(0))
    rev_spec = pdf.copy()
    contrib = contrib + np.where(diff[:, None], C.texture("Kd") / K.pi, T(0))
    pdf = pdf + np.where(diff, (1 - kw) * cos_wo / K.pi, T(0))
    rev_diff = np.where(diff, (1 - kw) * cos_wi / K.pi, T(0))
    return contrib * cos_wo[:, None], pdf, rev_spec, rev_diff, spec, diff


def phong_evaluate(C, sel):
    K, T, f, k = C.K, C.T, C.flow, C.K.k
    f.alive = sel.copy()
    C.put("contrib", sel, T(0)), C.put("pdf", sel, T(0)), C.put("revPdf", sel, T(0))
    cos_wi, n_, _ = _facing(C)
    cos_wo = dot(n_, C.wo0)
    C.put("cosWo", sel, cos_wo)
    f.note("cosWi", "abs", cos_wi, K.eps, forced=C.axis)
    f.leave(cos_wi <= K.eps)
    f.note("cosWo", "abs", cos_wo, K.eps, forced=C.axis)
    f.leave(cos_wo <= K.eps)
    a = f.alive.copy()
    contrib, pdf, rev_spec, rev_diff, _, _ = _phong_lobes(C, f, a, cos_wi, cos_wo, reflect(C.wi, n_), C.wo0, False)
    big = np.max(contrib, 1)
    f.note("MaxCoeff(contrib)", "mag", big, 1e-10)
    C.put("contrib", a, np.where((big < k(1e-10))[:, None], T(0), contrib))
    C.put("pdf", a, pdf)
    C.put("revPdf", a, rev_spec + rev_diff)


def phong_sample(C, sel):
    K, T, f, k = C.K, C.T, C.flow, C.K.k
    f.alive = sel.copy()
    cos_wi, n_, raw = _facing(C)
    f.note("|cosWi|", "abs", np.abs(raw), K.eps, forced=C.axis)
    C.ok[f.leave(np.abs(raw) < K.eps)] = False
    C.ok[f.leave((raw < 0) & ~C.twoSided)] = False
    kw, u = C.KsWeight, C.rnd[:, 0]
    expo = C.texture("expOrAlpha")[:, 0]
    R = reflect(C.wi, n_)
    diffuse = u > kw  # the first uniform picks the lobe and, rescaled, is the lobe's azimuth
    f.note("uDiscrete-KsWeight", "exact", u - kw, 0)
    g = np.where(diffuse, T(1), expo)
    axis = np.where(diffuse[:, None], n_, R)
    with np.errstate(all="ignore"):
        u0 = np.where(diffuse, (u - kw) / (1 - kw + k(1e-10)), u / (kw + k(1e-10)))
        cos_a = np.power(C.rnd[:, 1], 1 / (g + 1))
        sin_a = np.sqrt(1 - cos_a**2)
    phi = 2 * K.pi * u0
    b0, b1, _ = coordinate_system(axis, K)
    f.note("n.z", "exact", axis[:, 2], K.nzflip, where=diffuse)
    f.note("R.z", "abs", axis[:, 2], K.nzflip, where=~diffuse)
    wo = to_world(np.stack([sin_a * np.cos(phi), sin_a * np.sin(phi), cos_a], 1).astype(T), b0, b1, axis)
    cos_wo = dot(n_, wo)
    a = f.alive.copy()
    C.put("wo", a, wo), C.put("cosWo", a, cos_wo)
    f.note("cosWo", "abs", cos_wo, K.eps)
    C.ok[f.leave(cos_wo < K.eps)] = False
    a = f.alive.copy()
    contrib, pdf, rev_spec, rev_diff, spec, _ = _phong_lobes(C, f, a, cos_wi, cos_wo, R, wo, True)
    # the reverse density: the specular part replaces what the caller passed in, the diffuse part is ADDED -- with KsWeight == 0 onto the caller's value
    rev = np.where(spec, rev_spec, C.out["revPdf"]) + rev_diff
    C.put("pdf", a, pdf), C.put("revPdf", a, rev), C.put("contrib", a, contrib)
    f.note("pdf", "mag", pdf, 1e-10)
    C.ok[f.leave(pdf < k(1e-10))] = False
    with np.errstate(all="ignore"):
        C.put("contrib", f.alive, contrib / pdf[:, None])


def roughdielectric_evaluate(C, sel):
    K, T, f, k = C.K, C.T, C.flow, C.K.k
    f.alive = sel.copy()
    wi, wo, n, eta, inv_eta = C.wi, C.wo0, C.nrm, C.eta, C.invEta
    C.put("contrib", sel, T(0)), C.put("cosWo", sel, T(0)), C.put("pdf", sel, T(0)), C.put("revPdf", sel, T(0))
    cos_wi = dot(wi, n)
    f.note("|cosWi|", "abs", np.abs(cos_wi), K.eps, forced=C.axis)
    f.leave(np.abs(cos_wi) < K.eps)
    cos_wo = dot(wo, n)
    C.put("cosWo", f.alive, cos_wo)
    f.note("|cosWo|", "abs", np.abs(cos_wo), K.eps, forced=C.axis)
    f.leave(np.abs(cos_wo) < K.eps)
    f.note("cosWi*cosWo", "abs", cos_wi * cos_wo, 0)
    refl = cos_wi * cos_wo > 0
    e = np.where(cos_wi > 0, eta, inv_eta)  # the relative index seen from wi's side, and from wo's
    er = np.where(cos_wo > 0, eta, inv_eta)
    with np.errstate(all="ignore"):
        H = normalize(np.where(refl[:, None], wi + wo, wi + wo * e[:, None]))  # the half vector; for refraction the generalised one
    hn = dot(H, n)
    f.note("H.n", "abs", hn, 0)
    H = np.where((hn < 0)[:, None], -H, H)
    cos_hwi, cos_hwo = dot(wi, H), dot(wo, H)
    f.note("|cosHWi|", "abs", np.abs(cos_hwi), K.eps)
    f.leave(np.abs(cos_hwi) < K.eps)
    f.note("|cosHWo|", "abs", np.abs(cos_hwo), K.eps)
    f.leave(np.abs(cos_hwo) < K.eps)
    f.note("cosHWi*cosWi", "abs", cos_hwi * cos_wi, 0)
    f.leave(cos_hwi * cos_wi <= 0)
    f.note("cosHWo*cosWo", "abs", cos_hwo * cos_wo, 0)
    f.leave(cos_hwo * cos_wo <= 0)
    b0, b1, _ = coordinate_system(n, K)
    f.note("n.z", "exact", n[:, 2], K.nzflip)
    local_h = np.stack([dot(b0, H), dot(b1, H), dot(n, H)], 1)
    alp = C.texture("expOrAlpha")[:, 0]
    D = beckmann_d(local_h, alp, K)
    f.note("D", "underflow", D, 0)
    f.leave(~(D > 0))
    F, _, ct2 = fresnel(cos_hwi, eta, inv_eta, K)
    f.note("cosThetaTSqr", "abs", ct2, 0)
    G = beckmann_g1(alp, np.abs(cos_wi), K, f, "a(wi)-1.6") * beckmann_g1(alp, np.abs(cos_wo), K, f, "a(wo)-1.6")
    # the sampler draws its micro-normal from a widened lobe (Walter et al. 2007, section 5.3): alpha (1.2 - 0.2 sqrt|cos|)
    prob = local_h[:, 2] * beckmann_d(local_h, alp * (k(1.2) - k(0.2) * np.sqrt(np.abs(cos_wi))), K)
    f.note("prob", "mag", prob, 1e-20)
    f.leave(prob < k(1e-20))
    rev_prob = local_h[:, 2] * beckmann_d(local_h, alp * (k(1.2) - k(0.2) * np.sqrt(np.abs(cos_wo))), K)
    with np.errstate(all="ignore"):
        # reflection: f cos = F D G / (4 |cos wi|), dwh/dwo = 1 / (4 |wo.h|)
        s_r = np.abs(F * D * G / (4 * cos_wi))
        p_r = np.abs(prob * F / (4 * cos_hwo))
        q_r = np.abs(rev_prob * F / (4 * cos_hwi))
        # refraction: f cos = (1 - F) D G eta^2 |wi.h| |wo.h| / (|cos wi| (wi.h + eta wo.h)^2), dwh/dwo = eta^2 |wo.h| / (wi.h + eta wo.h)^2;
        # radiance (not importance) is scaled by 1 / eta^2 on the way through
        den, rden = cos_hwi + e * cos_hwo, cos_hwo + er * cos_hwi
        factor = np.where(C.adjoint, T(1), (1 / e) ** 2)
        s_t = np.abs(factor * ((1 - F) * D * G * e**2 * cos_hwi * cos_hwo) / (cos_wi * den**2))
        p_t = np.abs(prob * (1 - F) * (e**2 * cos_hwo) / den**2)
        q_t = np.abs(rev_prob * (1 - F) * (er**2 * cos_hwi) / rden**2)
    scalar, pdf, rev = np.where(refl, s_r, s_t), np.where(refl, p_r, p_t), np.where(refl, q_r, q_t)
    for name, q in (("scalar", scalar), ("pdf", pdf), ("revPdf", rev)):
        f.note(name + " underflow", "underflow", q, 0)
    a = f.alive
    C.put("contrib", a, np.where(refl[:, None], C.texture("Ks"), C.texture("Kt")) * scalar[:, None])
    C.put("pdf", a, pdf), C.put("revPdf", a, rev)


def roughdielectric_sample(C, sel):
    K, T, f, k = C.K, C.T, C.flow, C.K.k
    f.alive = sel.copy()
    wi, n, eta, inv_eta = C.wi, C.nrm, C.eta, C.invEta
    cos_wi = dot(wi, n)
    f.note("|cosWi|", "abs", np.abs(cos_wi), K.eps, forced=C.axis)
    C.ok[f.leave(np.abs(cos_wi) < K.eps)] = False
    alp = C.texture("expOrAlpha")[:, 0]
    local_h, m_pdf = sample_micronormal(C.rnd, alp * (k(1.2) - k(0.2) * np.sqrt(np.abs(cos_wi))), K)
    C.put("pdf", f.alive, m_pdf)
    b0, b1, _ = coordinate_system(n, K)
    f.note("n.z", "exact", n[:, 2], K.nzflip)
    H = to_world(local_h, b0, b1, n)
    cos_hwi = dot(wi, H)
    f.note("|cosHWi|", "abs", np.abs(cos_hwi), K.eps)
    C.ok[f.leave(np.abs(cos_hwi) < K.eps)] = False
    F, cos_t, ct2 = fresnel(cos_hwi, eta, inv_eta, K)
    f.note("cosThetaTSqr", "abs", ct2, 0)
    f.note("uDiscrete-F", "abs", C.u - F, 0, forced=(ct2 < -ABS_MARGIN) & (C.u < 1))  # under total internal reflection F is exactly 1
    refl = C.u <= F
    wo = np.where(refl[:, None], reflect(wi, H), refract(wi, H, cos_t, eta, inv_eta))
    C.put("wo", f.alive, wo)
    sides = dot(n, wo) * dot(n, wi)
    f.note("(n.wo)(n.wi)", "abs", sides, 0)
    C.ok[f.leave(np.where(refl, (F <= 0) | (sides <= 0), (F >= 1) | (cos_t == 0) | (sides >= 0)))] = False
    cos_hwo, cos_wo = dot(wo, H), dot(wo, n)
    e = np.where(cos_wi > 0, eta, inv_eta)
    er = np.where(cos_wo > 0, eta, inv_eta)
    rev_d = beckmann_d(local_h, alp * (k(1.2) - k(0.2) * np.sqrt(np.abs(cos_wo))), K)
    with np.errstate(all="ignore"):
        den, rden = cos_hwi + e * cos_hwo, cos_hwo + er * cos_hwi
        pdf = np.where(refl, np.abs(m_pdf * F / (4 * cos_hwo)), np.abs(m_pdf * (1 - F) * np.abs(e**2 * cos_hwo / den**2)))
        rev = np.where(refl, np.abs(F * rev_d * local_h[:, 2] / (4 * cos_hwi)), np.abs((1 - F) * rev_d * local_h[:, 2] * (er**2 * cos_hwi / rden**2)))
    a = f.alive.copy()
    C.put("pdf", a, pdf), C.put("cosWo", a, cos_wo)
    f.note("|cosWo|", "abs", np.abs(cos_wo), K.eps)
    C.ok[f.leave(np.abs(cos_wo) < K.eps)] = False
    f.note("revPdf underflow", "underflow", rev, 0)
    C.put("revPdf", f.alive, rev)
    f.note("|cosHWo|", "abs", np.abs(cos_hwo), K.eps)
    C.ok[f.leave(np.abs(cos_hwo) < K.eps)] = False
    f.note("pdf", "mag", pdf, 1e-20)
    C.ok[f.leave(pdf < k(1e-20))] = False
    f.note("cosHWi*cosWi", "abs", cos_hwi * cos_wi, 0)
    C.ok[f.leave(cos_hwi * cos_wi <= 0)] = False
    f.note("cosHWo*cosWo", "abs", cos_hwo * cos_wo, 0)
    C.ok[f.leave(cos_hwo * cos_wo <= 0)] = False
    D = beckmann_d(local_h, alp, K)
    G = beckmann_g1(alp, np.abs(cos_wi), K, f, "a(wi)-1.6") * beckmann_g1(alp, np.abs(cos_wo), K, f, "a(wo)-1.6")
    factor = np.where(C.adjoint, T(1), (1 / e) ** 2)
    colour = np.where(refl[:, None], C.texture("Ks"), C.texture("Kt") * factor[:, None])
    with np.errstate(all="ignore"):
        w = np.abs(D * G * cos_hwi / (m_pdf * np.abs(cos_wi)))  # f cos / pdf with the Fresnel factor and dwh/dwo cancelled against the lobe choice
    f.note("weight underflow", "underflow", w, 0)
    C.put("contrib", f.alive, colour * w[:, None])


EVALUATE = {LAMBERTIAN: lambertian_evaluate, PHONG: phong_evaluate, ROUGHDIELECTRIC: roughdielectric_evaluate}
SAMPLE = {LAMBERTIAN: lambertian_sample, PHONG: phong_sample, ROUGHDIELECTRIC: roughdielectric_sample}


def run(op, glossy, materials, bitmap_wh, bitmap_gamma, texels, case_ints, case_in, dtype=np.float64):
    """lmc_shade_probe's operation on its arguments, in `dtype`.  -> dict: ok [n] bool, out [n, 9] dtype (the words the operation did not write hold
    what went in), written [n, 9] bool, decisions (see decisive())"""
    T = np.dtype(dtype).type
    ints = np.asarray(case_ints, np.int64).reshape(-1, 3)
    tex = Textures(bitmap_wh, bitmap_gamma, texels)
    C = _Case(materials, tex, ints, case_in, T)
    n = C.n
    if op == OP_TEX:
        m = np.asarray(materials, np.float32)[ints[:, 0]]
        mi = m.view(np.int32)
        o = 2 + 6 * ints[:, 2]
        r = np.arange(n)
        ref = (mi[r, o].astype(np.int64), np.stack([m[r, o + 1], m[r, o + 2], m[r, o + 3]], 1), m[r, o + 4], m[r, o + 5])
        C.put("contrib", np.ones(n, bool), eval_tex(ref, C.st, tex, C.K))
    else:
        table = EVALUATE if op == OP_EVALUATE else SAMPLE
        types = C.type if glossy else np.zeros(n, np.int64)  # the Lambertian-only instantiation runs the Lambertian functions on any record
        for t, fn in table.items():
            sel = types == t
            if sel.any():
                fn(C, sel)
    out = np.zeros((n, 9), T)
    written = np.zeros((n, 9), bool)
    for q, s in OUT.items():
        out[:, s] = C.out[q].reshape(n, -1)
        written[:, s] = C.written[q][:, None]
    return dict(ok=C.ok.copy(), out=out, written=written, decisions=C.flow.decisions)


# ------------------------------------------------------------------------------------------------ bars
QUANTITIES = ("wo", "contrib", "cosWo", "pdf", "revPdf")


def rel_dev(a, b):
    """per case and output quantity [n, 5]: max |a - b| over the quantity's words / max |b| (0 where both vanish); a, b [n, 9]"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.zeros((len(a), len(QUANTITIES)))
    for j, q in enumerate(QUANTITIES):
        d = np.max(np.abs(a[:, OUT[q]] - b[:, OUT[q]]), 1)
        s = np.max(np.abs(b[:, OUT[q]]), 1)
        with np.errstate(all="ignore"):
            out[:, j] = np.where(d == 0, 0.0, d / s)
    return out


BAR_MARGIN = 4.0
# MEASURED[family][quantity]: the largest rel_dev of run(dtype=float32) from run(dtype=float64) over the CONDITIONED family of tests/shade_cases.py
# (seed and sizes as committed there), over the cases both precisions take the same way; measured by `python -m tests.shade_cases --measure`, which
# prints this table.  A float implementation must stay within BAR_MARGIN times it: the product's lpowf / lexpf / lsinf / lcosf are 1.5 - 2 ulp
# rather than numpy's correctly rounded ones, and the order of operations may legitimately differ.  A property of this file alone: nothing of the
# product enters the measurement.
MEASURED = {
    'cond_lambert_evaluate': {'wo': 0.00e+00, 'contrib': 1.18e-05, 'cosWo': 4.79e-07, 'pdf': 4.81e-07, 'revPdf': 4.66e-07},
    'cond_lambert_sample': {'wo': 4.99e-07, 'contrib': 1.27e-05, 'cosWo': 5.83e-08, 'pdf': 9.62e-08, 'revPdf': 4.33e-07},
    'cond_phong_evaluate': {'wo': 0.00e+00, 'contrib': 1.49e-04, 'cosWo': 2.50e-06, 'pdf': 1.49e-04, 'revPdf': 1.49e-04},
    'cond_phong_sample': {'wo': 3.34e-06, 'contrib': 1.43e-05, 'cosWo': 2.00e-05, 'pdf': 8.22e-05, 'revPdf': 8.22e-05},
    'cond_dielectric_evaluate': {'wo': 0.00e+00, 'contrib': 5.86e-05, 'cosWo': 5.99e-07, 'pdf': 5.03e-05, 'revPdf': 4.78e-05},
    'cond_dielectric_sample': {'wo': 5.80e-05, 'contrib': 2.76e-04, 'cosWo': 3.17e-04, 'pdf': 7.06e-04, 'revPdf': 3.58e-04},
    'cond_textures': {'wo': 0.00e+00, 'contrib': 4.09e-05, 'cosWo': 0.00e+00, 'pdf': 0.00e+00, 'revPdf': 0.00e+00},
}


def bars(family):
    return {q: BAR_MARGIN * v for q, v in MEASURED[family].items()}
