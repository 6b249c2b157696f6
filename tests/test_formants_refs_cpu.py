"""The references and bounds of tests/formants_ld_refs.py without a GPU: the conditions under which
test_formants_diff_gpu.py means something (FORMANTS.md, "Differential tests").  On every hard polynomial the numpy model
of the device iteration converges well inside its bound of iterations and meets the residual bound; the forward rule
8 delta <= separation admits the families it must and refuses the ones it must; the model sits inside delta and rho;
deliberately wrong root sets land outside.  On every frame shape a float64 evaluation of the decimator and the LPC sits
inside the long-double bounds, the bounds are small enough to mean something, and five wrong chains land outside."""
import numpy as np
import pytest

from . import formants_ld_refs as fl
from . import formants_refs as refs

POLYS = fl.hard_polys()
IDS = [p["label"] for p in POLYS]
SHAPES = fl.frame_shapes()


def by_label(label):
    return POLYS[IDS.index(label)]


# ---- roots -----------------------------------------------------------------------------------------------------------
def test_the_families_are_the_ones_listed():
    assert len(set(IDS)) == len(IDS)
    for k in (2, 4, 6):
        for fam in ("nearreal", "realpair", "pairpair"):
            assert "%s_1e-%d" % (fam, k) in IDS
    for label in ("double_real", "quad_real", "z_minus_0.9_pow8", "double_pair", "z16_minus_1", "z64_minus_1", "z63_plus_1",
                  "moduli_1e-3_to_1e3", "wilkinson10", "wilkinson20", "gauss10", "gauss32", "gauss64"):
        assert label in IDS
    for order in (16, 48, 64):
        assert "lpc%d_noise" % order in IDS and "lpc%d_two_sines" % order in IDS
    assert sorted({len(p["c"]) - 1 for p in POLYS if p["label"].startswith("wide64")}) == [64]
    assert sorted({p["c"][0] for p in POLYS if p["start"] is not None or p["mult"] is not None}) == [-0.37, 1.0, 3.0]
    z = np.abs(fl.analyse(by_label("moduli_1e-3_to_1e3"))["z"])
    assert z.min() <= 1.001e-3 and z.max() >= 0.999e3
    for p in POLYS:
        assert np.all(np.isfinite(p["c"])) and p["c"][0] != 0 and len(p["c"]) - 1 <= 64


@pytest.mark.parametrize("label", IDS)
def test_model_converges_in_half_the_bound_and_meets_the_residual_bound(label):
    p = by_label(label)
    a = fl.analyse(p)
    assert a["conv"] and a["its"] <= fl.MAX_ITER // 2, a["its"]
    r = fl.residual_ratio(p["c"], a["model"])
    print("%s: CPU model: %d iterations, worst |p(z)| / hb %.3f (allowed 4)" % (label, a["its"], r))
    assert r <= 4.0
    # the same yardstick as the existing test's
    for v in a["model"]:
        res, bound = refs.horner_bound(p["c"], v)
        assert res <= 4 * bound
    # the canonical form keeps it: a pair is an iterate and its mirror image, only a real root moves (by its imaginary part)
    canon, _, _ = fl.canonical_model(p["c"])
    fl.check_canonical(p["c"], canon)
    rc = fl.residual_ratio(p["c"], canon)
    print("%s: CPU model: canonical roots: worst |p(z)| / hb %.3f" % (label, rc))
    assert rc <= 4.0


def test_an_iterate_whose_choice_is_not_returned_looks_again():
    """wide64_seed201 has a pair at 0.63 +- 0.11i whose delta, 0.13, is larger than its distance to the next root: the
    iterates of its two members are not each other's nearest mirror images.  The rule as it was made both real at once,
    0.105 off their iterates and 6.4 of hb off the polynomial; a second round pairs them."""
    p = by_label("wide64_seed201")
    old, _, _ = fl.canonical_model(p["c"], rounds=False)
    new, _, _ = fl.canonical_model(p["c"])
    assert fl.residual_ratio(p["c"], old) > 4.0 and int(np.sum(old.imag == 0)) == 4
    assert fl.residual_ratio(p["c"], new) <= 1.0 and int(np.sum(new.imag == 0)) == 2 == p["nreal"]
    for q in POLYS:                                    # roots apart by more than their error settle in the first round: the same bits
        if fl.analyse(q)["kind"] == "forward":
            assert fl.canonical_model(q["c"], rounds=False)[0].tobytes() == fl.canonical_model(q["c"])[0].tobytes(), q["label"]


def test_the_forward_rule_admits_and_refuses_what_it_must():
    kinds = {p["label"]: fl.analyse(p)["kind"] for p in POLYS}
    forward = [k for k, v in kinds.items() if v == "forward"]
    assert len(forward) >= 20, forward
    for seed, _ in fl.WIDE_SEEDS:
        assert kinds["wide64_seed%d" % seed] == "forward"
    for seed, _ in fl.WIDE_REFUSED:                                    # delta / separation above 1: the discs overlap
        a = fl.analyse(by_label("wide64_seed%d" % seed))
        assert kinds["wide64_seed%d" % seed] == "residual" and float(np.max(a["delta"] / a["sep"])) > 0.125
    for k in (2, 4, 6):
        for fam in ("nearreal", "realpair", "pairpair"):
            a = fl.analyse(by_label("%s_1e-%d" % (fam, k)))
            assert a["kind"] == "forward"
            worst = float(np.max(a["delta"] / a["sep"]))
            print("%s_1e-%d: delta / separation %.2e" % (fam, k, worst))
            assert worst <= 7e-3                                       # far inside the rule's 1/8
            assert 0.5 * 10.0 ** -k <= float(np.min(a["sep"])) <= 2.5 * 10.0 ** -k   # the close roots stayed that close
    for label in ("double_real", "quad_real", "z_minus_0.9_pow8", "double_pair"):
        a = fl.analyse(by_label(label))
        assert a["kind"] == "cluster" and a["ok"], label              # 8 rho within the distance to the next distinct root
        assert all(8 * r <= g for r, g in zip(a["rho"], a["gap"]))
    for p in POLYS:                                                    # the references are what they claim to be
        a = fl.analyse(p)
        if a["kind"] == "forward":
            assert np.all(8 * a["cert"] <= a["delta"]) and np.all(8 * a["delta"] <= a["sep"])
            if p["nreal"] is not None:
                assert int(np.sum(a["z"].imag == 0)) == p["nreal"], p["label"]
            assert (len(a["z"]) - int(np.sum(a["z"].imag == 0))) % 2 == 0


@pytest.mark.parametrize("label", IDS)
def test_model_sits_inside_delta_and_rho(label):
    p = by_label(label)
    a = fl.analyse(p)
    if a["kind"] == "forward":
        r = fl.forward_ratio(a["model"], a)
        print("%s: CPU model: worst forward error / delta %.3f" % (label, r))
        assert r <= 1.0
        canon, _, _ = fl.canonical_model(p["c"])
        assert fl.forward_ratio(canon, a) <= 1.0
        assert fl.check_canonical(p["c"], canon) == int(np.sum(a["z"].imag == 0))
    elif a["kind"] == "cluster":
        ok, worst = fl.cluster_ok(a["model"], p, a)
        print("%s: CPU model: worst distance / rho %.3f" % (label, worst))
        assert ok
        canon, _, _ = fl.canonical_model(p["c"])
        assert fl.cluster_ok(canon, p, a)[0]
        assert (fl.check_canonical(p["c"], canon) - p["nreal"]) % 2 == 0
    else:
        assert label in ("wilkinson20",) + tuple("wide64_seed%d" % s for s, _ in fl.WIDE_REFUSED)


@pytest.mark.parametrize("label", [l for l in IDS if fl.analyse(by_label(l))["kind"] == "forward"])
def test_wrong_root_sets_land_outside(label):
    a = fl.analyse(by_label(label))
    z = a["z"].astype(np.complex128)
    assert fl.forward_ratio(z, a) <= 1.0
    # one root replaced by a copy of its nearest neighbour
    d = np.abs(z[:, None] - z[None, :])
    np.fill_diagonal(d, np.inf)
    w = z.copy()
    w[0] = z[np.argmin(d[0])]
    assert fl.forward_ratio(w, a) == np.inf
    # a pair (or, without one, a real root) with its real part off by 100 delta
    i = int(np.argmax(z.imag))
    w = z.copy()
    off = 100 * float(a["delta"][i])
    assert z[i].real + off != z[i].real
    w[i] = z[i] + off
    if z[i].imag > 0:
        j = int(np.argmin(np.abs(z - np.conj(z[i]))))
        w[j] = z[j] + off
    assert fl.forward_ratio(w, a) == np.inf
    # a real root given imag = 1e-9: outside its disc wherever delta < 1e-9 (everywhere but the real roots 1e-6 apart,
    # whose delta is 1.4e-9), and everywhere one exactly-real root fewer than the references have, which the GPU test counts
    real = np.nonzero(z.imag == 0)[0]
    if len(real):
        k = real[int(np.argmin(a["delta"][real]))]
        w = z.copy()
        w[k] = z[k] + 1e-9j
        assert int(np.sum(w.imag == 0)) != int(np.sum(a["z"].imag == 0))
        assert float(a["delta"][k]) < 1e-9 and fl.forward_ratio(w, a) == np.inf


def test_wrong_cluster_sets_land_outside():
    for label in ("double_real", "quad_real", "double_pair"):
        p = by_label(label)
        a = fl.analyse(p)
        z, _, _ = fl.canonical_model(p["c"])
        assert fl.cluster_ok(z, p, a)[0]
        (r, m), (s, k) = p["mult"][0], p["mult"][-1]
        w = z.copy()
        w[int(np.argmin(np.abs(z - r)))] = s                           # one of the m moved to another root
        assert not fl.cluster_ok(w, p, a)[0]
        w = z.copy()
        w[int(np.argmin(np.abs(z - r)))] += 100 * float(a["rho"][0])
        assert not fl.cluster_ok(w, p, a)[0]


def test_check_canonical_refuses_rows_that_are_not():
    p = by_label("nearreal_1e-4")
    z, _, _ = fl.canonical_model(p["c"])
    assert fl.check_canonical(p["c"], z) == 1
    nk = int(np.sum(z.imag >= 0))
    bad = []
    w = z.copy(); w[0] = complex(z[0].real, -0.0) if z[0].imag == 0 else np.conj(z[0]); bad.append(w)
    w = z.copy(); i = int(np.argmax(z.imag)); w[i] = complex(z[i].real, np.nextafter(z[i].imag, 1.0)); bad.append(w)
    w = z.copy(); w[:nk] = z[:nk][::-1]; bad.append(w)
    w = z.copy(); w[nk:] = z[nk:][::-1]; bad.append(w)
    for w in bad:
        with pytest.raises(AssertionError):
            fl.check_canonical(p["c"], w)
    with pytest.raises(AssertionError):
        fl.check_canonical(np.concatenate((p["c"], [0.0])), np.concatenate((z, [1e-300])))


def test_the_scale_prediction_of_the_model():
    """Without the division by c[0] the model's |p'|^2 leaves float64's range at c * 1e-160, c * 1e-200 and c * 1e200: the
    loop runs to its bound with iterates that are not finite, or (degree 5 at 1e-160, |p'|^2 subnormal) stops on a step of
    0 at points 1e12 of Horner's bound off; at 1e-100 it converges.  With the division every scale gives the iterates of c
    (a power of two: bit for bit)."""
    c, _ = refs.poly_from_roots(np.random.default_rng(6), 5, 1)
    z0, its0, conv0 = fl.aberth_model(c)
    assert conv0
    for s in (1e-160, 1e-200, 1e200):
        z, its, conv = fl.aberth_model(c * s, normalise=False)
        assert (not conv and its == fl.MAX_ITER and not np.all(np.isfinite(z))) or fl.residual_ratio(c * s, z) > 1e6
    z, its, conv = fl.aberth_model(c * 1e-100, normalise=False)
    assert conv and fl.residual_ratio(c * 1e-100, z) <= 4.0
    for s in (1e-160, 1e-200, 1e200, 3e150, -1e-160):
        z, its, conv = fl.aberth_model(c * s)
        assert conv and its <= fl.MAX_ITER // 2 and fl.residual_ratio(c * s, z) <= 4.0
    for k in (-600, -100, 100, 600):
        z, its, conv = fl.aberth_model(c * 2.0 ** k)
        assert conv and its == its0 and z.tobytes() == z0.tobytes()


# ---- frames ----------------------------------------------------------------------------------------------------------
def test_the_shapes_are_the_ones_listed():
    assert len({s["label"] for s in SHAPES}) == len(SHAPES)
    for sh in SHAPES:
        n, down = fl.shape_n(sh), sh["down"]
        nd = -(-n // down)
        assert (sh["nfr"] - 1) * sh["hop"] + sh["nwind"] == nd         # the last frame ends on decimated sample ceil(n / down) - 1
        assert sh["nfr"] >= 4 and sh["order"] < sh["nwind"]
    one = [s for s in SHAPES if s["down"] == 1]
    assert sorted(s["pre"] for s in one) == [0, 1] and all(fl.shape_n(s) == 61 and (s["nwind"], s["hop"], s["order"]) == (12, 7, 4) for s in one)
    asym = {(s["down"], s["L"]) for s in SHAPES if not s["sym"]}
    assert {(2, 41), (3, 61), (4, 81), (8, 161)} <= asym and {1, 3, 7} <= {L for _, L in asym}
    for down in (3, 4):
        assert {fl.shape_n(s) % down for s in SHAPES if s["down"] == down} == set(range(down))
    assert all(17 <= s["nwind"] <= 40 for s in SHAPES if s["down"] > 1 and not s["sym"])
    assert [(s["down"], s["nwind"], s["hop"], s["order"]) for s in SHAPES if s["sym"]] == [(4, 276, 138, 10)]
    assert any(s["nwind"] == s["order"] + 1 and s["order"] == 16 for s in SHAPES)
    assert {s["dtype"] for s in SHAPES} == {"float32", "float64", "int16"}
    for sh in SHAPES:
        x, h, w = fl.shape_inputs(sh)
        assert x.dtype == np.dtype(sh["dtype"]) and len(x) == fl.shape_n(sh) and np.array_equal(x, np.round(x.astype(np.float64)))
        if h is not None and not sh["sym"] and len(h) > 1:
            assert not np.allclose(h, h[::-1])


@pytest.mark.parametrize("sh", SHAPES, ids=[s["label"] for s in SHAPES])
def test_float64_chain_sits_inside_the_bounds_and_wrong_chains_outside(sh):
    x, h, wind = fl.shape_inputs(sh)
    ref = fl.frame_refs(sh)
    order = sh["order"]
    worst = 0.0
    for (a, bound), (v, _) in zip(ref, fl.frame_inputs(sh, x, h, wind, dtype=np.float64)):
        assert np.isfinite(bound) and 0 < bound <= 1e-8, bound         # the cap of test_glottal_refs_cpu.py
        worst = max(worst, fl.gl.ratio(fl.lpc_f64(v, order)[1:], a[1:], bound))
    print("%s: float64 chain: worst |a - reference| / bound %.4f, bounds %.1e .. %.1e"
          % (sh["label"], worst, min(b for _, b in ref), max(b for _, b in ref)))
    assert worst <= 1.0
    y_ref, _ = fl.decimated(x, sh["pre"], sh["down"], h)
    read = np.zeros(len(y_ref), dtype=bool)
    for f in fl.FRAMES_CHECKED:
        f = f % sh["nfr"]
        read[f * sh["hop"]:f * sh["hop"] + sh["nwind"]] = True
    for wrong in fl.WRONG_CHAINS:
        y, _ = fl.decimated(x, sh["pre"], sh["down"], h, wrong)
        if not np.any((y != y_ref) & read):                            # no mistake at this shape (one tap, no remainder, ...)
            continue
        out = 0.0
        for (a, bound), (v, _) in zip(ref, fl.frame_inputs(sh, x, h, wind, wrong, dtype=np.float64)):
            out = max(out, fl.gl.ratio(fl.lpc_f64(v, order)[1:], a[1:], bound))
        print("%s: %s: %.1e of the bound" % (sh["label"], wrong, out))
        assert out > 1.0, wrong


def test_every_wrong_chain_is_a_mistake_at_several_shapes():
    count = dict.fromkeys(fl.WRONG_CHAINS, 0)
    for sh in SHAPES:
        x, h, wind = fl.shape_inputs(sh)
        y_ref, _ = fl.decimated(x, sh["pre"], sh["down"], h)
        last = slice((sh["nfr"] - 1) * sh["hop"], None)
        for wrong in fl.WRONG_CHAINS:
            y, _ = fl.decimated(x, sh["pre"], sh["down"], h, wrong)
            count[wrong] += bool(np.any(y[last] != y_ref[last]))      # it shows in the last frame, at the end of the signal
    assert all(v >= 3 for v in count.values()), count
