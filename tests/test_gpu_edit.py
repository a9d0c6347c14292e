"""Image editing through the engine (include/glass.h "Image editing"), on the mini StyleGAN2 + mini CLIP of tests/glass_models.py, P = 8,
batch 4, noise_mode 0 unless said otherwise.

(a) a direction source, views off: F[:, 0] recomputed by edit_ref's float32 twin from the pass's own features, source rows and set;
(b) the same with 3 crop views, fixed and redrawn boxes at two generations: the source rows change exactly when the boxes do;
(c) the source image generated from row r makes candidate r score exactly 0 in every view;
(d) the anchor against float64 of the dlatents (map_latents + the truncation rule of tests/dlatent_ref.py) in z, w and w+ and with psi 0.7;
    the anchor row itself gives 0; the own-column and the folded layout of F;
(e) chunks, offsets and a population scored whole give the same bits with both features on;
(f) feature off: the bits of an engine that never heard of it;
(g) one device-search step with the anchor column (n_obj = 3);
(h) call-order refusals by name;
(i) one `run` end to end with --edit-latent.

Bars: the general one of tests/test_gpu_edit_ops.py against float64; the number of elements whose bits differ from the float32 twin is logged.

Measured on an MI355X: F[:, 0], the per-entry columns, the per-view cosines and the anchor distances all have the float32 twin's bits (errors
against float64 2e-8 to 2e-7, a quarter of their bars); the source rows are unit_rows of encode_generated's feature bit for bit; in (c) row 5
scores 0 in its three views, its three columns and F[5, 0] (-0.0), while every other row has a column above 1e-4."""
import os
import pickle

import numpy as np
import pytest
import torch

import dlatent_ref as DR
import edit_ref as E
import glass_models as M
from clip_glass_amd import engine as G
from clip_glass_amd import synth
from util import diag

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("GLASS_EMULATE")), reason="launches the library's own kernels: no emulated form")]
F32 = np.float32
C = M.CONFIGS["mini"]
P, BS, L, EMB, R = 8, 4, C["latent"], C["clip"][5], 32
N_LAT = 2 * len(C["channels"])


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _same_bits(name, got, want):
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    diag("[edit-engine] %-60s bit-exact: %d / %d elements differ" % (name, int(bad.sum()), bad.size))
    assert not bad.any(), "%s: %d elements differ, first at %s" % (name, int(bad.sum()), np.argwhere(bad)[0])


def _bar(name, got, ref64, ref32):
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    tol = E.bar(ref64, ref32)
    err = np.abs(got - ref64)
    twin = int((_bits(got) != _bits(ref32)).sum())
    diag("[edit-engine] %-60s max err %.3e  bar %.3e  max|ref| %.3e  bits differ from the twin: %d / %d" % (name, err.max(), tol, np.abs(ref64).max(), twin, got.size))
    assert np.isfinite(got).all() and (err <= tol).all(), "%s: max err %.3e, bar %.3e" % (name, err.max(), tol)


@pytest.fixture(scope="module")
def sd():
    return M.make_state("mini", 0)


def make(sd, *, use_d=True, noise_mode=0, views=0, fixed=False, space="z", psi=1.0, anchor=False, anchor_lambda=0.0, chunk=0, search=False,
         finalize=True):
    n_obj = G.edit_n_obj(0, use_d, False, anchor, anchor_lambda)
    e = G.Engine(C["channels"][::-1], latent_size=L, mapping_layers=C["mapping"], batch_size=BS, use_discriminator=use_d, n_obj=n_obj, max_pop=P,
                 chunk=chunk, clip=C["clip"], noise_mode=noise_mode, noise_seed=3, clip_views=views, clip_view_fixed=fixed, latent_space=space,
                 truncation_psi=psi, anchor=anchor, anchor_lambda=anchor_lambda)
    if search:
        e.set_search("nsga2", P, -10.0, 10.0, seed=1)
    e.load_state(sd)
    e.load_tensor("dlatent_avg", synth.dlatent_avg(L, 0))
    if finalize:
        e.finalize()
    return e


def rows(space="z", seed=6):
    x = np.random.default_rng(seed).standard_normal((P, L)).astype(F32)
    if space == "w+":
        x = (x[:, None, :] + 0.3 * np.random.default_rng(seed + 1).standard_normal((P, N_LAT, L))).astype(F32).reshape(P, -1)
    return x


def directions(T=3, seed=4):
    rng = np.random.default_rng(seed)
    return E.unit_rows(rng.standard_normal((T, EMB)).astype(F32), F32), np.array([1.0, -0.5, 2.0, 0.25], F32)[:T]


def source_image(seed=8):
    """A smooth random picture in [-1, 1] (an 8 x 8 grid of normals, upsampled)."""
    g = np.random.default_rng(seed).standard_normal((3, 8, 8))
    return np.clip(np.kron(g, np.ones((4, 4))) * 0.5, -1, 1).astype(F32)


# ---- (a), (b) -----------------------------------------------------------------------------------------------------------------------
def test_directional_similarity_is_the_twin_of_the_pass_own_features(sd):
    e = make(sd)
    dirs, w = directions()
    img = source_image()
    e.set_targets(dirs, w)
    e.set_direction_source(img)
    Fv = e.evaluate(rows())
    feat, src = e.details(P)["features"], e.last_direction_source()
    assert src.shape == (1, EMB)
    raw = e.encode_generated(img[None])
    _same_bits("source row == unit_rows(encode_generated(image))", src, E.unit_rows(raw, F32))
    r64, r32 = E.cosine_set_dir(feat[:, None], dirs, w, src), E.cosine_set_dir(feat[:, None], dirs, w, src, dt=F32)
    e.set_direction_source(img)                 # (encode_generated went through the head: score again for the set's details)
    F2 = e.evaluate(rows())
    _same_bits("a second pass", F2, Fv)
    _bar("views off: -F[:, 0]", -Fv[:, 0], r64[2], r32[2])
    _bar("views off: per-entry columns", e.set_details(P), r64[1], r32[1])
    assert np.abs(Fv[:, 0]).max() > 1e-3
    # the plain set on the same engine is another number: the source is really subtracted
    e.set_direction_source(None)
    F0 = e.evaluate(rows())
    assert np.abs(F0[:, 0] - Fv[:, 0]).max() > 1e-3
    _same_bits("the hinge column does not move", F0[:, 1], Fv[:, 1])
    e.close()


@pytest.mark.parametrize("fixed", [True, False])
def test_directional_similarity_with_three_views(sd, fixed):
    e = make(sd, views=3, fixed=fixed)
    dirs, w = directions()
    e.set_targets(dirs, w)
    e.set_direction_source(source_image())
    seen = []
    for gen in (0, 1):
        Fv = e.evaluate(rows(), generation=gen)
        vd, src = e.view_details(P), e.last_direction_source()
        assert src.shape == (3, EMB)
        r64 = E.cosine_set_dir(vd["features"], dirs, w, src)
        r32 = E.cosine_set_dir(vd["features"], dirs, w, src, dt=F32)
        tag = "3 views %s gen %d" % ("fixed" if fixed else "redrawn", gen)
        _bar(tag + ": -F[:, 0]", -Fv[:, 0], r64[2], r32[2])
        _bar(tag + ": entry 0 per view", vd["sims"], r64[0], r32[0])
        _bar(tag + ": per-entry columns", e.set_details(P), r64[1], r32[1])
        np.testing.assert_allclose(np.linalg.norm(src.astype(np.float64), axis=1), 1.0, atol=1e-6)
        seen.append((vd["boxes"].copy(), src.copy()))
    (b0, s0), (b1, s1) = seen
    _same_bits("view 0 (the whole image) keeps its source row", s1[0], s0[0])
    if fixed:
        assert np.array_equal(b0, b1)
        _same_bits("fixed boxes: the same source rows at both generations", s1, s0)
    else:
        assert not np.array_equal(b0[1:], b1[1:])
        for v in (1, 2):
            assert np.array_equal(b0[v], b1[v]) == np.array_equal(_bits(s0[v]), _bits(s1[v])), "view %d: rows and boxes must change together" % v
        assert (_bits(s0[1:]) != _bits(s1[1:])).any()
    e.close()


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------
def test_the_source_generated_from_a_row_scores_that_row_zero(sd):
    e = make(sd, views=3)
    x = rows()
    dirs, w = directions()
    e.set_targets(dirs, w)
    r = 5
    img01 = e.generate(x)[r]
    e.set_direction_source(2.0 * img01 - 1.0)
    Fv = e.evaluate(x)
    vd, ss = e.view_details(P), e.set_details(P)
    diag("[edit-engine] source = image of row %d: its views score %s, its columns %s, F %s" % (r, vd["sims"][r], ss[r], Fv[r, 0]))
    assert not vd["sims"][r].any() and not ss[r].any() and Fv[r, 0] == 0
    others = np.delete(np.arange(P), r)
    assert (np.abs(ss[others]).max(axis=1) > 1e-4).all()
    e.close()


# ---- (d) ------------------------------------------------------------------------------------------------------------------------------
def _dlatents(e, x, space, psi):
    """[P, n_lat, L] float32: map_latents (z), then the truncation rule of tests/dlatent_ref.py."""
    if space == "z":
        d = np.repeat(e.map_latents(x)[:, None], N_LAT, 1)
    elif space == "w":
        d = np.repeat(x[:, None], N_LAT, 1)
    else:
        d = x.reshape(P, N_LAT, L)
    lp = DR.layer_psi(N_LAT, psi, None)
    if lp is not None:
        t = torch.from_numpy(np.ascontiguousarray(d))
        avg = torch.as_tensor(synth.dlatent_avg(L, 0)).float()
        d = torch.lerp(avg.expand_as(t), t, torch.tensor(lp).view(1, -1, 1).expand_as(t)).numpy()
    return np.ascontiguousarray(d, F32)


@pytest.mark.parametrize("space,psi", [("z", 1.0), ("w", 1.0), ("w+", 1.0), ("z", 0.7), ("w+", 0.7)])
def test_anchor_distance_and_its_column(sd, space, psi):
    e = make(sd, space=space, psi=psi, anchor=True)
    x = rows(space)
    target = np.random.default_rng(4).standard_normal(EMB).astype(F32)
    e.set_target(target)
    e.set_anchor(x[2])
    Fv = e.evaluate(x)
    assert Fv.shape == (P, 3)
    d, det = e.last_anchor(P), e.details(P)
    dl = _dlatents(e, x, space, psi)
    tag = "anchor %s psi %.1f" % (space, psi)
    _bar(tag, d, E.latent_anchor(dl, dl[2]), E.latent_anchor(dl, dl[2], dt=F32))
    assert d[2] == 0 and (d[np.arange(P) != 2] > 1e-3).all()
    _same_bits(tag + ": F's last column is d", Fv[:, 2], d)
    _same_bits(tag + ": F's first column is -sim", Fv[:, 0], -det["sim"])
    _same_bits(tag + ": F's hinge", Fv[:, 1], np.maximum(F32(1) - det["dis"], F32(0)))
    # another truncation after set_anchor: the stored anchor follows it
    if psi == 1.0 and space != "w":
        e.set_truncation(0.7)
        e.evaluate(x)
        d7 = e.last_anchor(P)
        dl7 = _dlatents(e, x, space, 0.7)
        _bar(tag + " -> psi 0.7 after set_anchor", d7, E.latent_anchor(dl7, dl7[2]), E.latent_anchor(dl7, dl7[2], dt=F32))
        assert d7[2] == 0 and np.abs(d7 - d).max() > 1e-3
    e.close()
    # folded: no column; F[:, 0] = fmaf(lambda, d, -sim) (lambda 0.5: the product is exact, the fold one float32 addition)
    e = make(sd, space=space, psi=psi, anchor=True, anchor_lambda=0.5)
    e.set_target(target)
    e.set_anchor(x[2])
    Ff = e.evaluate(x)
    assert Ff.shape == (P, 2)
    _same_bits(tag + ": folded distances", e.last_anchor(P), d)
    _same_bits(tag + ": folded F[:, 0]", Ff[:, 0], (F32(0.5) * d + (-e.details(P)["sim"])).astype(F32))
    _same_bits(tag + ": folded hinge", Ff[:, 1], Fv[:, 1])
    e.close()


# ---- (e) ------------------------------------------------------------------------------------------------------------------------------
def test_chunks_offsets_and_the_whole_population_agree(sd):
    dirs, w = directions()
    img, x = source_image(), rows()
    out = []
    for chunk in (0, 4):
        e = make(sd, noise_mode=1, views=3, anchor=True, chunk=chunk)
        e.set_targets(dirs, w)
        e.set_direction_source(img)
        e.set_anchor(x[1])
        whole = e.evaluate(x, generation=2)
        halves = np.concatenate([e.evaluate(x[:4], generation=2, first_minibatch=0), e.evaluate(x[4:], generation=2, first_minibatch=1)])
        _same_bits("chunk %d: two slices == the population scored whole" % chunk, halves, whole)
        out.append(whole)
        e.close()
    _same_bits("chunk 4 == chunk 0", out[1], out[0])
    assert out[0].shape == (P, 3) and (out[0][:, 2] > 0).sum() == P - 1


# ---- (f) ------------------------------------------------------------------------------------------------------------------------------
def test_feature_off_returns_the_bits_of_today(sd):
    x = rows()
    dirs, w = directions()
    plain = M.make_engine("mini", sd, batch_size=BS, max_pop=P, noise_mode=0)        # created as every existing test creates it
    plain.set_targets(dirs, w)
    F0, s0 = plain.evaluate(x), plain.set_details(P)
    plain.close()
    e = make(sd)                                  # the longer struct, zeros in the new fields
    assert e.cfg.anchor == 0 and e.cfg.anchor_lambda == 0.0
    e.set_targets(dirs, w)
    _same_bits("zeros in the new fields", e.evaluate(x), F0)
    e.set_direction_source(source_image())
    e.evaluate(x)
    e.set_direction_source(None)                  # on and off again
    _same_bits("a source set and cleared", e.evaluate(x), F0)
    _same_bits("a source set and cleared: the set's columns", e.set_details(P), s0)
    e.close()


# ---- (g) ------------------------------------------------------------------------------------------------------------------------------
def test_one_device_search_step_with_the_anchor_column(sd):
    e = make(sd, noise_mode=1, anchor=True, search=True)
    dirs, w = directions()
    X0 = rows()
    e.set_targets(dirs, w)
    e.set_direction_source(source_image())
    e.set_anchor(X0[0])
    e.search_init(X0)
    p0 = e.search_read("X", "F")
    assert p0["F"].shape == (P, 3)
    i0 = int(np.argwhere((_bits(p0["X"]) == _bits(X0[0])).all(axis=1))[0, 0])
    assert p0["F"][i0, 2] == 0                   # the anchor's own row, wherever survival put it
    e.search_step(1)
    a = e.search_read("X", "F", "off_X", "off_F", "counts")
    Fe = e.evaluate(a["off_X"], generation=1)
    _same_bits("search_step's offspring F == evaluate of the read-back rows", a["off_F"], Fe)
    _same_bits("its last column == last_anchor", Fe[:, 2], e.last_anchor(P))
    assert np.isfinite(a["F"]).all() and (a["off_F"][:, 2] > 0).all()
    # the survivors' rows of F are rows of the merged F
    merged = np.concatenate([p0["F"], a["off_F"]])
    for row in a["F"]:
        assert (_bits(merged) == _bits(row)).all(axis=1).any()
    e.close()


# ---- (h) ------------------------------------------------------------------------------------------------------------------------------
def test_call_order_refusals(sd):
    e = make(sd, anchor=True, finalize=False)
    with pytest.raises(RuntimeError, match=r"set_anchor: finalize\(\) first"):
        e.set_anchor(rows()[0])
    with pytest.raises(RuntimeError, match=r"set_direction_source: finalize\(\) first"):
        e.set_direction_source(source_image())
    e.finalize()
    e.set_target(np.ones(EMB, F32))
    with pytest.raises(RuntimeError, match=r"set_anchor\(\) first"):
        e.evaluate(rows())
    with pytest.raises(RuntimeError, match="no anchor is set"):
        e.last_anchor(P)
    e.set_anchor(rows()[0])
    e.evaluate(rows())
    with pytest.raises(RuntimeError, match="no direction source is set"):
        e.last_direction_source()
    e.set_direction_source(source_image())
    with pytest.raises(RuntimeError, match=r"set_targets\(\) first"):
        e.evaluate(rows())                        # a single target is no set of directions
    e.set_targets(*directions())
    assert e.evaluate(rows()).shape == (P, 3)
    with pytest.raises(ValueError, match=r"must be \[3, 32, 32\]"):
        e.set_direction_source(np.zeros((3, 16, 16), F32))
    e.close()
    e = make(sd)
    with pytest.raises(RuntimeError, match="created without an anchor"):
        e.set_anchor(rows()[0])
    e.close()
    v = make(sd, views=3)
    v.set_targets(*directions())
    v.set_direction_source(source_image())
    with pytest.raises(RuntimeError, match="made by the first evaluate"):
        v.last_direction_source()
    v.close()


# ---- (i) ------------------------------------------------------------------------------------------------------------------------------
def test_run_cli_edits_a_latent(tmp_path, monkeypatch):
    """`python -m clip_glass_amd.run --edit-latent ROW.npy --source-text ...`: two NSGA-II generations on mini-sized synthetic weights (sized
    as tests/test_gpu_engine.py::test_run_cli_end_to_end sizes its run; the text features are given, there is no vocabulary on every machine).
    Three objectives: similarity, discriminator, anchor."""
    from clip_glass_amd import run
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "mini_problem.npz")))
    src_text = np.random.default_rng(12).standard_normal(EMB).astype(F32)
    extra = dict(channels=C["channels"], dim_z=L, mapping_layers=C["mapping"], clip_geometry=C["clip"], clip_text_geometry=dict(width=64, layers=2),
                 target_features=g["text_features"], source_text_features=src_text,
                 problem_args=dict(n_var=L, n_obj=2, n_constr=L, xl=-10, xu=10))
    row = np.random.default_rng(13).standard_normal(L).astype(F32)
    row[0] = 11.5                                 # outside the config's +-10: the bounds are widened to contain the source
    np.save(str(tmp_path / "row.npy"), row)
    seen = []
    inner = run.GenerationProblem._evaluate

    def recording(self, x, out, *a, **k):
        inner(self, x, out, *a, **k)
        seen.append((np.array(x), np.array(out["F"]), float(np.max(self.xu))))
    monkeypatch.setattr(run.GenerationProblem, "_evaluate", recording)
    argv = ["--config", "StyleGAN2_ffhq_d", "--generations", "2", "--save-each", "1", "--tmp-folder", str(tmp_path), "--weights", "synthetic:0",
            "--clip-weights", "synthetic:0", "--pop-size", "8", "--edit-latent", str(tmp_path / "row.npy"), "--source-text", "a face",
            "--edit-sigma", "0.2"]
    res = run.main(argv, extra_config=extra)
    assert np.atleast_2d(res.X).shape[1] == L and np.atleast_2d(res.F).shape[1] == 3
    for f in ("source.jpg", "genetic-it-1.jpg", "genetic-it-final.jpg", "genetic_result", "ls_result", "output.jpg", "F-similarity-discriminator.jpg",
              "F-similarity-anchor.jpg", "F-discriminator-anchor.jpg"):
        assert os.path.getsize(os.path.join(str(tmp_path), f)) > 0, f
    assert not os.path.exists(os.path.join(str(tmp_path), "F.jpg"))
    X0, F0, xu = seen[0]                          # generation 0
    assert X0.shape == (8, L) and F0.shape == (8, 3) and xu == 11.5
    np.testing.assert_array_equal(X0[0].astype(F32), row)
    assert F0[0, 2] == 0 and (F0[1:, 2] > 0).all()          # the source row is its own anchor
    assert 0.1 < (X0[1:, 1:] - row[1:]).std() < 0.3 and (X0 <= 11.5).all() and (X0 >= -10).all()
    d = pickle.load(open(os.path.join(str(tmp_path), "genetic_result"), "rb"))
    Fr, Xr = np.atleast_2d(d["F"]), np.atleast_2d(d["X"])
    assert Fr.shape[1] == 3
    i = int(np.argmin(Fr[:, 2]))                   # nothing dominates the one candidate at distance 0: the source survives on the front
    assert Fr[i, 2] == 0 and np.array_equal(Xr[i].astype(F32), row)
