"""numpy restatement of the twenty PPO-diagnostics words (include/catan_hip_nn.h: catan_ppo_diag) and the input builder of the tests that
compare against it.  A helper, not a test; it never imports the package's own torch form.

The sums are fp64 of the fp32 inputs.  The decisions behind words 6..9 are taken in numpy fp32 with the loss kernel's expressions -
exp(logp - old) in fp32, the fp32 normaliser with its + 1e-4f, lo / hi, inside, vin, l1 >= l2 - because those words count what the loss
did.  An fp32 exp or division may differ in the last bit between implementations, so the builder keeps every row at least 1e-4 away
from each decision boundary (it replaces the few that are closer by a fixed row): the integer words are then comparable exactly, and no
row is left out of any comparison."""
import numpy as np

WORDS = 20
SUM_WORDS = (0, 1, 2, 3, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18)
MAX_WORDS = (4, 5, 19)
INTEGER_WORDS = (0, 1, 6, 7, 8, 9, 18)
SCALAR_WORDS = (16, 17, 18, 19)
F32 = np.float32

SAFE_ROW = dict(d=0.05, adv=1.0, v=0.1, vp=0.0, ret=1.0)
MARGIN = 1e-4
MAX_REPLACED = 0.02


def _decisions(logp, old_logp, adv, v, vp, ret, clip, norm):
    """the loss kernel's fp32 expressions -> dict of fp32 / bool arrays"""
    logp, old_logp, adv, v, vp, ret = (np.asarray(x, dtype=F32) for x in (logp, old_logp, adv, v, vp, ret))
    clip = F32(clip)
    if norm is not None:
        mean, den = F32(norm[0]), F32(norm[1]) + F32(1e-4)
        vp, ret = (vp - mean) / den, (ret - mean) / den
    lo, hi = F32(1.0) - clip, F32(1.0) + clip
    ratio = np.exp(logp - old_logp)
    s1 = ratio * adv
    s2 = np.minimum(np.maximum(ratio, lo), hi) * adv
    inside = (ratio >= lo) & (ratio <= hi)
    dv = v - vp
    vc = vp + np.minimum(np.maximum(dv, -clip), clip)
    e1, e2 = v - ret, vc - ret
    l1, l2 = e1 * e1, e2 * e2
    vin = (dv >= -clip) & (dv <= clip)
    for x in (ratio, s1, s2, dv, vc, l1, l2):
        assert x.dtype == F32
    return dict(ratio=ratio, lo=lo, hi=hi, s1=s1, s2=s2, inside=inside, dv=dv, l1=l1, l2=l2, vin=vin, clip=clip)


def reference_words(logp, old_logp, adv, v, vp, ret, clip, norm=None, entropy=None, grad_norm=None, max_grad_norm=0.0):
    """One call into a zeroed block -> (words float64 [20], abs_terms float64 [20] = the sum of |term| behind every sum word).
    entropy / grad_norm: fp32 scalars or None (their words stay 0)."""
    k = _decisions(logp, old_logp, adv, v, vp, ret, clip, norm)
    logp, old_logp, v, vp, ret = (np.asarray(x, dtype=F32).astype(np.float64) for x in (logp, old_logp, v, vp, ret))
    if norm is not None:
        mean, den = float(F32(norm[0])), float(F32(norm[1])) + 1e-4
        vp, ret = (vp - mean) / den, (ret - mean) / den
    d = logp - old_logp
    e, e0 = ret - v, ret - vp
    w, a = np.zeros(WORDS), np.zeros(WORDS)
    terms = {2: -d, 3: np.expm1(d) - d, 10: ret, 11: ret * ret, 12: e, 13: e * e, 14: e0, 15: e0 * e0}
    for i, t in terms.items():
        w[i], a[i] = t.sum(), np.abs(t).sum()
    w[0], w[1] = d.size, 1
    w[4], w[5] = np.maximum(d, 0.0).max(), np.maximum(-d, 0.0).max()
    w[6] = np.count_nonzero(~k["inside"])
    w[7] = np.count_nonzero(~k["inside"] & (k["s1"] > k["s2"]))
    w[8] = np.count_nonzero(~k["vin"])
    w[9] = np.count_nonzero((k["l2"] > k["l1"]) & ~k["vin"])
    if entropy is not None:
        w[16] = float(F32(entropy)); a[16] = abs(w[16])
    if grad_norm is not None:
        g = F32(grad_norm)
        w[17] = float(g); a[17] = abs(w[17])
        w[18] = 1.0 if (max_grad_norm > 0 and g > F32(max_grad_norm)) else 0.0
        w[19] = float(g)
    return w, a


def combine(refs):
    """several calls into one block: [(words, abs_terms), ...] -> (words, abs_terms)"""
    w = np.sum([r[0] for r in refs], axis=0)
    for i in MAX_WORDS:
        w[i] = max(r[0][i] for r in refs)
    return w, np.sum([r[1] for r in refs], axis=0)


def assert_words(got, ref, abs_terms, untouched=()):
    """integer and maximum words exactly; sum words within 1e-10 * sum|term| (a reordered fp64 sum of B terms is off by at most
    B * 2^-53 * sum|term|, and B <= 2^18 here: 2.9e-11)"""
    got = np.asarray(got, dtype=np.float64)
    for i in range(WORDS):
        if i in untouched:
            continue
        if i in INTEGER_WORDS or i in MAX_WORDS:
            assert got[i] == ref[i], (i, got[i], ref[i])
        else:
            assert abs(got[i] - ref[i]) <= 1e-10 * abs_terms[i], (i, got[i], ref[i], abs_terms[i])


def build_inputs(B, seed, clip, norm=None):
    """-> dict of fp32 arrays logp, old_logp, adv, v, vp, ret (vp, ret denormalised when norm = (mean, std)), and `replaced`.
    Three rows in four move by d ~ N(0, 0.15) (both clip sides populated), the fourth by N(0, 2e-3) (the scale a fresh learner starts from)."""
    rng = np.random.RandomState(seed)
    old = -rng.uniform(0.05, 3.0, B)
    d = rng.normal(0.0, 0.15, B) * np.where(rng.randint(0, 4, B) == 0, 2e-3 / 0.15, 1.0)
    adv = rng.normal(0.0, 1.0, B)
    v = rng.normal(0.0, 0.5, B)
    vp = v + rng.normal(0.0, 0.15, B)
    ret = rng.normal(0.0, 0.7, B)

    if norm is not None:                     # the kernel reads vp and ret denormalised
        vp, ret = norm[0] + norm[1] * vp, norm[0] + norm[1] * ret
    old = old.astype(F32)
    x = dict(logp=(old + d.astype(F32)).astype(F32), old_logp=old, adv=adv.astype(F32), v=v.astype(F32), vp=vp.astype(F32), ret=ret.astype(F32))
    k = _decisions(x["logp"], x["old_logp"], x["adv"], x["v"], x["vp"], x["ret"], clip, norm)
    big = np.maximum(k["l1"], k["l2"])
    near = (np.abs(k["ratio"] - k["lo"]) < MARGIN) | (np.abs(k["ratio"] - k["hi"]) < MARGIN)
    near |= np.abs(np.abs(k["dv"]) - k["clip"]) < MARGIN
    near |= ~k["vin"] & (np.abs(k["l1"] - k["l2"]) <= MARGIN * big)       # (inside the value clip the outcome of l1 >= l2 decides nothing)
    near |= np.abs(x["adv"]) < 1e-3
    s = SAFE_ROW                             # written as the kernel reads it, whatever the normaliser
    x["logp"][near] = x["old_logp"][near] + F32(s["d"])
    for name in ("adv", "v", "vp", "ret"):
        x[name][near] = F32(s[name])
    x["replaced"] = int(near.sum())
    assert x["replaced"] <= MAX_REPLACED * B, (B, seed, x["replaced"])
    return x


# the cases of the kernel test: (B, seed).  B = 1: one workgroup, gridDim 1; 257: a partial second workgroup; 65 537: every workgroup
# populated plus one wrap of the grid stride; 200 003: an odd size near the config-3 minibatch (204 800)
CASES = ((1, 11), (257, 12), (65537, 13), (200003, 14))
SETTINGS = tuple((clip, norm) for clip in (0.2, 0.1) for norm in (None, (150.0, 150.0)))
