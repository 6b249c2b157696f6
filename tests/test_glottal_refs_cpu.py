"""The long-double references and bounds of tests/glottal_ld_refs.py without a GPU: on every shape of the sweep of
test_glottal_diff_gpu.py a float64 evaluation -- the restatement of glottal_refs.py with a numpy emulation of the
integrator's 256-block scan -- stays inside every stage bound, the bounds are tight enough for that sweep to mean
something, and a set of deliberately wrong evaluations each leaves its stage bound on at least one case.  Also the
float64 emulations test_glottal_diff_gpu.py has no use for but the mutations need."""
import numpy as np
import pytest

from . import glottal_ld_refs as ld
from . import glottal_refs as refs


# ---- float64 evaluations, with the switches of the mutations ---------------------------------------------------------
def scan256(v, leak, power_off=0, right_aligned_tail=False):
    """v[j] += leak v[j-1] as the blocked scan of GLOTTAL.md: 256 blocks of B = ceil(len / 256) from a zero carry, a chain
    over the block ends, leak^(j - s + 1) times the carry added; the powers by repeated multiplication.
    power_off: the carry's power is off by that much.  right_aligned_tail: the partial last block takes the powers of a
    full block's last samples."""
    m = len(v)
    B = -(-m // 256)
    pw = [1.0]
    for _ in range(2 * B + 1):
        pw.append(pw[-1] * leak)
    out = [float(t) for t in v]
    ends, carry = [0.0] * 256, [0.0] * 256
    for t in range(256):
        prev = 0.0
        for j in range(t * B, min(t * B + B, m)):
            prev = out[j] + leak * prev
            out[j] = prev
        ends[t] = prev
    c = 0.0
    for q in range(256):
        carry[q] = c
        ln = min(B, m - q * B)
        if ln > 0:
            c = ends[q] + pw[ln] * c
    for t in range(1, 256):
        s, e = t * B, min(t * B + B, m)
        shift = power_off + (B - (e - s) if right_aligned_tail and s < e else 0)
        for j in range(s, e):
            out[j] = out[j] + pw[j - s + 1 + shift] * carry[t]
    return np.array(out)


def frame64(xf, b, hw, pt, pg, leak, n_it, highpass=refs.highpass, fir=refs.fir, integ=scan256, lpc=refs.lpc,
            ramp=lambda y0, P: np.linspace(-y0, y0, P)):
    """glottal_refs.frame with every stage replaceable"""
    P = pt + 1
    y = highpass(xf, b)
    u = np.concatenate([ramp(y[0], P), y])
    Hg = lpc(y * hw, 1)
    y = fir(Hg, u)[P:]
    for _ in range(n_it):
        Hvt = lpc(y * hw, pt)
        g = integ(fir(Hvt, u), leak)[P:]
        Hg = lpc(g * hw, pg)
        y = integ(fir(Hg, u), leak)[P:]
    Hvt = lpc(y * hw, pt)
    dfull = fir(Hvt, u)
    return integ(dfull, leak)[P:], dfull[P:], Hvt, Hg


def ola64(g, dg, wind, hop, n, skip_first=False):
    """the gather of GLOTTAL.md: per sample its covering frames in ascending order, divided where the window sum is > 0"""
    nfr, nwind = g.shape
    glot, dglot = np.zeros(n), np.zeros(n)
    for s in range(n):
        fa, fb = max(0, -(-(s - nwind + 1) // hop)), min(s // hop, nfr - 1)
        a = d = ws = 0.0
        for f in range(fa + (1 if skip_first else 0), fb + 1):
            j = s - f * hop
            a, d, ws = a + g[f, j] * wind[j], d + dg[f, j] * wind[j], ws + wind[j]
        if ws > 0:
            a, d = a / ws, d / ws
        glot[s], dglot[s] = a, d
    return glot, dglot


def fir_last_tap_dropped(h, u):
    return refs.fir(h[:-1], u) if len(h) > 1 else refs.fir(h, u)        # (an order-0 filter has no tap to spare)


def highpass_half_up(xf, b):
    """glottal_refs.highpass with hp = floor(L/2 - 1 + 0.5)"""
    xf = np.asarray(xf, dtype=np.float64)
    n, L = len(xf), len(b)
    hp = max(int(np.floor(L / 2 - 1 + 0.5)), 0)
    xz = np.concatenate([xf, np.zeros(hp)])
    return np.array([np.dot(b[:min(L - 1, i + hp) + 1], xz[i + hp - min(L - 1, i + hp):i + hp + 1][::-1]) for i in range(n)])


def lpc_last_product_dropped(v, p):
    r = refs.autocorr(v, p)
    n = len(v)
    return refs.levinson(r - np.array([v[n - 1] * v[n - 1 - k] if k < n else 0.0 for k in range(p + 1)]), p)


def check64(case, n_its=(0, 1, 2, 3), **ops):
    xf, b, hw = ld.case_inputs(case)
    nwind, L, pt, pg, leak, _ = case
    used_leak = ops.pop("leak", leak)
    return ld.check_frame(lambda n_it: frame64(xf, b, hw, pt, pg, used_leak, n_it, **ops), xf, b, hw, pt, pg, leak, n_its, key=case)


# ---- the reference meets its own bounds, and the bounds are worth meeting ---------------------------------------------
def test_long_double_is_wider_than_float64():
    assert np.finfo(ld.LD).eps <= 2.0 ** -63


_CHECKED = {}


def checked(case):
    """check64 of the whole chain of a case, computed once"""
    if case not in _CHECKED:
        _CHECKED[case] = check64(case)
    return _CHECKED[case]


@pytest.mark.parametrize("case", ld.FRAME_CASES, ids=ld.case_id)
def test_float64_evaluation_stays_within_every_stage_bound(case):
    ratios, caps = checked(case)
    print(ld.case_id(case), " ".join("%s %.3f" % kv for kv in sorted(ratios.items())))
    assert set(ratios) == {"gc0", "gc", "vt", "dg", "g"}
    assert all(r <= 1.0 for r in ratios.values()), ratios


@pytest.mark.parametrize("case", ld.FRAME_CASES, ids=ld.case_id)
def test_bounds_are_tight_enough_for_the_sweep_to_mean_something(case):
    """The dg and g bounds are <= 1e-10 of the case's largest |value| and every single-stage LPC bound is <= 1e-8 (every
    bound is finite, and > 0 where its reference is not 0: check_frame asserts that itself).  Where the seeded input of a
    case missed the LPC cap the input changed, not the cap: another seed (glottal_ld_refs.SEED_SALT), and for two cases that
    no seed of the coloured noise brought under it, white noise (WHITE_CASE, LIMITS_CASE: the figures are there)."""
    ratios, caps = checked(case)
    print(ld.case_id(case), " ".join("cap_%s %.2e" % kv for kv in sorted(caps.items())))
    assert caps["dg"] <= 1e-10 and caps["g"] <= 1e-10, caps
    assert caps["lpc"] <= 1e-8, caps


def test_the_stages_agree_with_the_float64_restatement():
    """the long-double functions compute what glottal_refs.py computes (loosely: this guards the formulas, not the rounding)"""
    case = (240, 8, 15, 6, 0.99, "hann")
    xf, b, hw = ld.case_inputs(case)
    y, e_y = ld.highpass(xf, b)
    assert np.max(np.abs(y.astype(np.float64) - refs.highpass(xf, b))) <= 1e-13 * np.max(np.abs(y))
    u, e_u = ld.padded_input(xf, b, 16)
    u64 = np.concatenate([np.linspace(-float(y[0]), float(y[0]), 16), refs.highpass(xf, b)])
    assert np.max(np.abs(u.astype(np.float64) - u64)) <= 1e-13 * np.max(np.abs(y))
    h = refs.lpc(xf * hw, 15)
    assert np.max(np.abs(ld.levinson(ld.autocorr(xf * hw, 15), 15, ld.LD).astype(np.float64) - h)) <= 1e-9
    f, ef = ld.fir(h, u, e_u)
    assert np.max(np.abs(f.astype(np.float64) - refs.fir(h, u64))) <= 1e-12 * np.max(np.abs(f))
    i, ei = ld.integ(f, ef, 0.99, ld.scan_roundings(len(u)))
    assert np.max(np.abs(i.astype(np.float64) - refs.integ(refs.fir(h, u64), 0.99))) <= 1e-12 * np.max(np.abs(i))
    # P = 1 is [-y0], the last element of a longer ramp is y0 itself
    assert ld.preramp(0.3, 0.0, 1)[0].tolist() == [-ld.LD(0.3)] and ld.preramp(0.3, 0.0, 7)[0][-1] == ld.LD(0.3)
    assert ld.hp_delay(1) == 0 and ld.hp_delay(2) == 0 and ld.hp_delay(7) == 2 and ld.hp_delay(9) == 4 and ld.hp_delay(8) == 3


def lpc_sweep():
    return [(p, n) for p in ld.LPC_ORDERS for n in ld.lpc_nwinds(p)] + [(8, 33)]


@pytest.mark.parametrize("order,nwind", lpc_sweep())
def test_float64_lpc_stays_within_the_lag_bound(order, nwind):
    x, hop = ld.lpc_case_signal(order, nwind)
    for wind in (None, np.hamming(nwind)):
        for q in (0, 3):                                               # the frames test_glottal_diff_gpu.py checks
            v = x[q * hop:q * hop + nwind] if wind is None else x[q * hop:q * hop + nwind] * wind
            r, bnd = ld.check_lpc_row(refs.lpc(v, order), v, order)
            print("order %d nwind %d %s frame %d: error / bound %.3f, bound %.2e" % (order, nwind, "bare" if wind is None else "hamming", q, r, bnd))
            assert r <= 1.0 and bnd <= 1e-8


def ola_rows(nwind, hop, n, seed):
    nfr = len(refs.frame_starts(n, nwind, hop))
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nfr, nwind)), rng.standard_normal((nfr, nwind))


@pytest.mark.parametrize("hop", [1, 13, 63, 64, 67])
@pytest.mark.parametrize("wname", ["hanning", "hamming"])
def test_float64_overlap_add_stays_within_its_bound(hop, wname):
    nwind, n = 64, 389
    wind = getattr(np, wname)(nwind)
    g, dg = ola_rows(nwind, hop, n, hop)
    glot, dglot = ola64(g, dg, wind, hop, n)
    want = refs.ola(np.zeros(n), nwind, hop, None, None, wind, 0, 0, 0, 0, frames=[(g[q], dg[q], None, None) for q in range(len(g))])
    assert glot.tobytes() == want[0].tobytes() and dglot.tobytes() == want[1].tobytes()      # the emulation is the restatement
    ratios, ws = ld.check_ola(glot, dglot, g, dg, wind, hop, n)
    print("hop %d %s: %s" % (hop, wname, ratios))
    assert all(r <= 1.0 for r in ratios.values()), ratios
    assert not glot[ws == 0].any() and not dglot[ws == 0].any()
    cover = (len(g) - 1) * hop + nwind
    assert cover < n and not ws[cover:].any()
    if wname == "hanning":                                             # sample 0 sees a zero end point only; at hop 63 so do the joins
        assert ws[0] == 0 and (hop != 63 or (ws[63] == 0 and ws[126] == 0))
        assert hop != 67 or not ws[64:67].any()
    else:
        assert ws[0] > 0


# ---- mutations: each must leave a stage bound on at least one case ----------------------------------------------------
SMALL = [c for c in ld.FRAME_CASES if c[0] <= 276 and c[2] <= 16]
MUTATIONS = {
    "carry power off by one": dict(integ=lambda v, leak: scan256(v, leak, power_off=-1)),
    "partial last block with the full block's power": dict(integ=lambda v, leak: scan256(v, leak, right_aligned_tail=True)),
    "last FIR tap dropped": dict(fir=fir_last_tap_dropped),
    "hp rounded half up": dict(highpass=highpass_half_up),
    "last product of a lag dropped": dict(lpc=lpc_last_product_dropped),
    "leak narrowed to float32": None,
    "pre-ramp step 2 y0 / P": dict(ramp=lambda y0, P: -y0 + np.arange(P) * (2 * y0 / P)),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutation_leaves_a_stage_bound(name):
    caught = {}
    for case in SMALL:
        ops = MUTATIONS[name] if MUTATIONS[name] is not None else dict(leak=float(np.float32(case[4])))
        ratios, _ = check64(case, n_its=(0, 1), **ops)
        if max(ratios.values()) > 1.0:
            caught[ld.case_id(case)] = max(ratios, key=ratios.get)
    print(name, caught)
    assert caught, name
    if name == "last product of a lag dropped":                       # invisible under a window that ends in a zero
        assert all(not cid.endswith("hann") for cid in caught)


def test_mutation_overlap_add_skips_the_first_covering_frame():
    nwind, n, hop = 64, 389, 13
    wind = np.hamming(nwind)
    g, dg = ola_rows(nwind, hop, n, 5)
    ratios, _ = ld.check_ola(*ola64(g, dg, wind, hop, n, skip_first=True), g, dg, wind, hop, n)
    assert min(ratios.values()) > 1.0, ratios
