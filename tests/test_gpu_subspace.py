"""Latent space "sub" through the engine (include/glass.h "Subspace latent space"): expand_latents against the float64 rule
(tests/subspace_ref.py), the pass pinned bit for bit to the w+ engine's pass on the expanded rows (which the w+ parity tests of
tests/test_gpu_dlatents.py pin to the reference), chunks and slices, the latent anchor, the device search, the refusals, run.py, and
the untouched default pass."""
import os
import pickle

import numpy as np
import pytest

import glass_models as M
import subspace_ref as S
from clip_glass_amd import subspace, synth
from clip_glass_amd.engine import Engine, edit_n_obj
from util import diag

pytestmark = pytest.mark.gpu
F32 = np.float32


def _engine(name, sd, avg=None, *, P=8, use_d=True, noise_mode=2, noise_seed=0, chunk=0, finalize=True, n_obj=None, **kw):
    c = M.CONFIGS[name]
    e = Engine(c["channels"][::-1], latent_size=c["latent"], mapping_layers=c["mapping"], batch_size=4, use_discriminator=use_d,
               n_obj=(2 if use_d else 1) if n_obj is None else n_obj, max_pop=P, chunk=chunk, clip=c["clip"], noise_mode=noise_mode,
               noise_seed=noise_seed, **kw)
    e.load_state(sd)
    if avg is not None:
        e.load_tensor("dlatent_avg", avg)
    if finalize:
        e.finalize()
    return e


def _space(name, K, groups, seed=0, P=8):
    """One subspace of a network: layer_group, basis [K][L] (0.3 N(0, 1): steps of the size of a dlatent's spread), a per-layer base,
    coefficient rows [P][G K]."""
    c = M.CONFIGS[name]
    L, n_lat = c["latent"], 2 * len(c["channels"])
    lg = S.layer_groups(n_lat)[groups]
    G = int(lg.max()) + 1
    rng = np.random.RandomState(40 + seed)
    return dict(lg=lg, G=G, K=K, L=L, n_lat=n_lat, basis=(0.3 * rng.normal(size=(K, L))).astype(F32), base=rng.normal(size=(n_lat, L)).astype(F32),
                rows=rng.normal(size=(P, G * K)).astype(F32))


@pytest.fixture(scope="module")
def nets():
    out = {}
    for name in ("mini", "mid"):
        c = M.CONFIGS[name]
        out[name] = dict(sd=M.make_state(name, 0), avg=synth.dlatent_avg(c["latent"], 0), planes=M.noise_planes(name, 7, 0, 2),
                         target=M.make_target(np.ones((8, c["clip"][5]), F32), seed=3))
    return out


def _sub_engine(name, net, sp, **kw):
    e = _engine(name, net["sd"], net["avg"], latent_space="sub", subspace_shape=(sp["G"], sp["K"]), **kw)
    e.set_subspace(sp["lg"], sp["basis"], sp["base"])
    return e


def _all_outputs(e, x, planes):
    F = e.evaluate(x, noise=planes)
    det = e.details(x.shape[0])
    return dict(F=F, features=det["features"], dis=det["dis"], img=e.generate(x, noise=planes))


def _same(a, b):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ---- 1. expand_latents ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,groups", [("mini", 5, "two_frozen_ends"), ("mini", 32, "per_layer"), ("mid", 16, "split_frozen_middle"),
                                           ("mid", 64, "one")])
def test_expand_latents_matches_the_rule(nets, name, K, groups):
    net, sp = nets[name], _space(name, K, groups)
    e = _sub_engine(name, net, sp, use_d=False)
    assert e.latent_row() == (sp["G"] * K, sp["n_lat"])
    c3 = sp["rows"].reshape(8, sp["G"], K)
    for psi, cutoff in ((1.0, None), (0.5, 3)):
        e.set_truncation(psi, cutoff)
        got = e.expand_latents(sp["rows"])
        ref, bar = S.expand(c3, sp["lg"], sp["basis"], sp["base"], psi=psi, cutoff=cutoff, avg=net["avg"])
        ok, worst, n_bad = S.within(got, ref, bar)
        diag("[subspace] expand %s K%d %s psi %.1f: worst err / bar %.3f" % (name, K, groups, psi, worst))
        assert got.shape == (8, sp["n_lat"], sp["L"]) and got.dtype == F32
        assert ok, "psi %.1f: %d elements outside the bar (worst ratio %.3f)" % (psi, n_bad, worst)
        np.testing.assert_array_equal(e.expand_latents(sp["rows"][5:6])[0], got[5])
    e.close()


def test_expand_latents_in_the_other_spaces(nets):
    net = nets["mini"]
    L, n_lat = 32, 8
    z = synth.latents(1, 8, L).astype(F32)
    e = _engine("mini", net["sd"], net["avg"], use_d=False)
    w = e.map_latents(z)
    np.testing.assert_array_equal(e.expand_latents(z), np.repeat(w[:, None], n_lat, 1))
    np.testing.assert_array_equal(e.expand_latents(z[:3]), np.repeat(w[:3, None], n_lat, 1))
    e.close()
    e = _engine("mini", net["sd"], net["avg"], use_d=False, latent_space="w")
    np.testing.assert_array_equal(e.expand_latents(w), np.repeat(w[:, None], n_lat, 1))
    e.close()
    wp = (np.repeat(w[:, None], n_lat, 1) + synth.normal(12, "w_plus8", (8, n_lat, L), 0.3)).astype(F32)
    e = _engine("mini", net["sd"], net["avg"], use_d=False, latent_space="w+")
    np.testing.assert_array_equal(e.expand_latents(wp.reshape(8, -1)), wp)
    e.set_truncation(0.5, 3)                       # truncated: the lerp towards the average on the first three layers, the rest as given
    t = e.expand_latents(wp.reshape(8, -1))
    np.testing.assert_array_equal(t[:, 3:], wp[:, 3:])
    assert np.abs(t[:, :3] - (net["avg"] + 0.5 * (wp[:, :3].astype(np.float64) - net["avg"]))).max() < 1e-5
    e.close()


# ---- 2. the pass in sub is the w+ pass on the expanded rows ------------------------------------------------------------------
@pytest.mark.parametrize("name,use_d,K,groups", [("mini", True, 6, "two_frozen_ends"), ("mid", False, 16, "split_frozen_middle")])
def test_pass_equals_the_w_plus_pass_on_the_expanded_rows(nets, name, use_d, K, groups):
    net, sp = nets[name], _space(name, K, groups, seed=1)
    e = _sub_engine(name, net, sp, use_d=use_d)
    e.set_target(net["target"])
    ew = _engine(name, net["sd"], net["avg"], use_d=use_d, latent_space="w+")
    ew.set_target(net["target"])
    for psi, cutoff in ((1.0, None), (0.5, 3)):
        e.set_truncation(psi, cutoff)
        out = _all_outputs(e, sp["rows"], net["planes"])
        wp = e.expand_latents(sp["rows"]).reshape(8, -1)
        assert np.isfinite(out["F"]).all() and len(set(out["F"][:, 0].tolist())) > 1
        _same(out, _all_outputs(ew, wp, net["planes"]))
    e.close()
    ew.close()


# ---- 3. identity basis -------------------------------------------------------------------------------------------------------
def test_identity_basis_is_w_plus(nets):
    net = nets["mini"]
    L, n_lat = 32, 8
    wp = synth.normal(13, "w_plus_id", (8, n_lat, L), 1.0).astype(F32)
    e = _engine("mini", net["sd"], net["avg"], latent_space="sub", subspace_shape=(n_lat, L))
    e.set_subspace(np.arange(n_lat), np.eye(L, dtype=F32), np.zeros((n_lat, L), F32))
    e.set_target(net["target"])
    assert e.latent_row() == (n_lat * L, n_lat)
    np.testing.assert_array_equal(e.expand_latents(wp.reshape(8, -1)), wp)
    ew = _engine("mini", net["sd"], net["avg"], latent_space="w+")
    ew.set_target(net["target"])
    _same(_all_outputs(e, wp.reshape(8, -1), net["planes"]), _all_outputs(ew, wp.reshape(8, -1), net["planes"]))
    e.close()
    ew.close()


# ---- 4. chunks and slices -------------------------------------------------------------------------------------------------------
def test_chunks_and_slices(nets):
    net, sp = nets["mini"], _space("mini", 6, "two_frozen_ends", seed=2, P=16)
    Fs = []
    for chunk in (4, 16):
        e = _sub_engine("mini", net, sp, P=16, noise_mode=1, noise_seed=77, chunk=chunk, truncation_psi=0.5, truncation_cutoff=3)
        e.set_target(net["target"])
        Fs.append(e.evaluate(sp["rows"], generation=2))
        if chunk == 16:
            whole = e.evaluate(sp["rows"][:8], generation=2)
            parts = [e.evaluate(sp["rows"][4 * m:4 * m + 4], generation=2, first_minibatch=m) for m in range(2)]
            np.testing.assert_array_equal(np.concatenate(parts), whole)
            np.testing.assert_array_equal(whole, Fs[-1][:8])
        e.close()
    assert np.isfinite(Fs[0]).all() and len(set(Fs[0][:, 0].tolist())) > 1
    np.testing.assert_array_equal(Fs[0], Fs[1])


# ---- 5. the latent anchor ----------------------------------------------------------------------------------------------------------
def test_anchor_is_the_distance_in_w(nets):
    net, sp = nets["mini"], _space("mini", 6, "two_frozen_ends", seed=3)
    n_obj = edit_n_obj(0, False, False, True, 0.0)
    e = _sub_engine("mini", net, sp, use_d=False, n_obj=n_obj, anchor=True)
    e.set_target(net["target"])
    e.set_anchor(np.zeros(sp["G"] * sp["K"], F32))            # the source is the zero row: its dlatents are `base`
    rows = sp["rows"].copy()
    rows[0] = 0
    F = e.evaluate(rows, noise=net["planes"])
    d = e.last_anchor(8)
    assert d[0] == 0.0 and (d[1:] > 0).all()
    np.testing.assert_array_equal(F[:, -1], d)
    ew = _engine("mini", net["sd"], net["avg"], use_d=False, n_obj=n_obj, anchor=True, latent_space="w+")
    ew.set_target(net["target"])
    ew.set_anchor(sp["base"].reshape(-1))
    Fw = ew.evaluate(e.expand_latents(rows).reshape(8, -1), noise=net["planes"])
    np.testing.assert_array_equal(ew.last_anchor(8), d)
    np.testing.assert_array_equal(Fw, F)
    # a new subspace recomputes the stored anchor, as set_truncation does
    e.set_subspace(sp["lg"], sp["basis"], sp["base"] + F32(1))
    e.evaluate(rows, noise=net["planes"])
    assert e.last_anchor(8)[0] == 0.0
    e.close()
    ew.close()


# ---- 6. device search ---------------------------------------------------------------------------------------------------------------
def _search_engine(net, algorithm, use_d, islands=0):
    sp = _space("mini", 8, "two_frozen_ends", seed=4, P=8 * max(islands, 1))        # G K = 16
    assert sp["G"] * sp["K"] == 16
    c = M.CONFIGS["mini"]
    e = Engine(c["channels"][::-1], latent_size=c["latent"], mapping_layers=c["mapping"], batch_size=4, use_discriminator=use_d,
               n_obj=2 if use_d else 1, max_pop=8 * max(islands, 1), clip=c["clip"], noise_mode=1, noise_seed=3, latent_space="sub",
               subspace_shape=(sp["G"], sp["K"]))
    e.set_search(algorithm, 8, -10.0, 10.0, seed=1)
    if islands:
        e.set_search_islands(islands, 2, 1)
    e.load_state(net["sd"])
    e.finalize()
    e.set_target(net["target"])
    return e, sp


@pytest.mark.parametrize("algorithm,use_d", [("ga", False), ("nsga2", True), ("cmaes", False)])
def test_device_search(nets, algorithm, use_d):
    e, sp = _search_engine(nets["mini"], algorithm, use_d)
    with pytest.raises(RuntimeError, match=r"set_subspace\(\) first"):
        e.search_init_cma(np.zeros(16)) if algorithm == "cmaes" else e.search_init(sp["rows"])
        e.search_step(1)
    e.set_subspace(sp["lg"], sp["basis"], sp["base"])
    if algorithm == "cmaes":
        e.search_init_cma(np.zeros(16), None, 1.0)
    else:
        e.search_init(sp["rows"])
    up0 = e.latent_uploads()
    for gen in (1, 2, 3):
        e.search_step(gen)
        assert e.latent_uploads() == up0          # no latent row crosses to the device after generation 0
        r = e.search_read("off_X", "off_F")
        assert r["off_X"].shape == (8, 16) and np.isfinite(r["off_F"]).all()
        np.testing.assert_array_equal(e.evaluate(r["off_X"], generation=gen), r["off_F"])
        up0 = e.latent_uploads()                  # (the check's own evaluate uploaded its rows)
    e.close()


def test_device_search_island_pair(nets):
    e, sp = _search_engine(nets["mini"], "ga", False, islands=2)
    e.set_subspace(sp["lg"], sp["basis"], sp["base"])
    e.search_init(sp["rows"])
    up0 = e.latent_uploads()
    for gen in (1, 2):
        e.search_step(gen)
    assert e.latent_uploads() == up0
    r = e.search_read("X", "F", islands=True)
    assert r["X"].shape == (2, 8, 16) and np.isfinite(r["F"]).all() and len(set(r["F"][..., 0].reshape(-1).tolist())) > 1
    e.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(nets):
    net, sp = nets["mini"], _space("mini", 6, "two_frozen_ends")
    e = _engine("mini", net["sd"], net["avg"], latent_space="sub", subspace_shape=(sp["G"], sp["K"]))
    e.set_target(net["target"])
    for call in (lambda: e.evaluate(sp["rows"], noise=net["planes"]), lambda: e.generate(sp["rows"], noise=net["planes"]),
                 lambda: e.expand_latents(sp["rows"])):
        with pytest.raises(RuntimeError, match=r"set_subspace\(\) first"):
            call()
    with pytest.raises(RuntimeError, match="finalized"):
        e.set_subspace_shape(2, 6)
    with pytest.raises(RuntimeError, match="group 1 is empty"):
        e.set_subspace(np.zeros(8, np.int32), sp["basis"], sp["base"])
    with pytest.raises(ValueError, match=r"basis \[6, 32\]"):
        e.set_subspace(sp["lg"], sp["basis"][:5], sp["base"])
    e.set_subspace(sp["lg"], sp["basis"], sp["base"])
    for bad in (np.zeros((8, 32), F32), sp["rows"][:, :-1], sp["rows"][0]):
        with pytest.raises(ValueError, match=r"\[P, 12\]"):
            e.evaluate(bad, noise=net["planes"])          # refused in Python: the library never sees the short rows
        with pytest.raises(ValueError, match=r"\[P, 12\]"):
            e.expand_latents(bad)
    assert np.isfinite(e.evaluate(sp["rows"], noise=net["planes"])).all()
    e.close()
    ea = _engine("mini", net["sd"], net["avg"], use_d=False, n_obj=2, anchor=True, latent_space="sub", subspace_shape=(sp["G"], sp["K"]))
    with pytest.raises(RuntimeError, match=r"set_subspace\(\) first"):
        ea.set_anchor(np.zeros(12, F32))
    ea.close()
    with pytest.raises(ValueError, match="subspace_shape"):
        _engine("mini", net["sd"], finalize=False, latent_space="sub")
    with pytest.raises(ValueError, match="subspace_shape belongs"):
        _engine("mini", net["sd"], finalize=False, latent_space="w+", subspace_shape=(1, 4))
    e = _engine("mini", net["sd"], finalize=False)
    with pytest.raises(RuntimeError, match="latent space is not sub"):
        e.set_subspace_shape(1, 4)                          # the space comes first
    e.set_latent_space("sub")
    for G, K, msg in ((1, 0, "components must be at least 1"), (1, 33, "latent_size 32"), (9, 4, "n_lat 8"), (0, 4, "groups must be at least 1")):
        with pytest.raises(RuntimeError, match=msg):
            e.set_subspace_shape(G, K)
    with pytest.raises(RuntimeError, match="set_subspace_shape"):
        e.finalize()                                         # sub without a shape
    e.close()
    b = M.BIGGAN_CONFIGS["bg_mini"]
    geo = dict(layers=b["layers"], attention_pos=b["attention_pos"], ch=b["ch"], z_dim=b["z_dim"], num_classes=b["num_classes"])
    eb = Engine([], batch_size=4, max_pop=8, clip=b["clip"], biggan=geo)
    with pytest.raises(RuntimeError, match="BigGAN"):
        eb.set_subspace_shape(1, 4)
    eb.close()
    with pytest.raises(RuntimeError, match="StyleGAN2"):
        Engine([], batch_size=4, max_pop=8, clip=b["clip"], biggan=geo, latent_space="sub", subspace_shape=(1, 4))


# ---- 8. run.py -------------------------------------------------------------------------------------------------------------------------
def _run_cli(tmp, monkeypatch, *more, config="StyleGAN2_ffhq_d", n_obj=2, **extra_kw):
    from clip_glass_amd import run
    c = M.CONFIGS["mini"]
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "mini_problem.npz")))
    extra = dict(channels=c["channels"], dim_z=c["latent"], mapping_layers=c["mapping"], clip_geometry=c["clip"],
                 clip_text_geometry=dict(width=64, layers=2), target_features=g["text_features"],
                 problem_args=dict(n_var=c["latent"], n_obj=n_obj, n_constr=c["latent"], xl=-10, xu=10), **extra_kw)
    seen = []
    inner = getattr(run.GenerationProblem._evaluate, "inner", run.GenerationProblem._evaluate)

    def recording(self, x, out, *a, **k):
        inner(self, x, out, *a, **k)
        seen.append((np.array(x), np.array(out["F"])))
    recording.inner = inner
    monkeypatch.setattr(run.GenerationProblem, "_evaluate", recording)
    os.makedirs(tmp, exist_ok=True)
    argv = ["--config", config, "--generations", "2", "--save-each", "1", "--tmp-folder", tmp, "--weights", "synthetic:0", "--clip-weights",
            "synthetic:0", "--pop-size", "8", "--latent-space", "sub", "--subspace-components", "8", "--subspace-layers", "0-3,4-7",
            "--subspace-samples", "256"] + list(more)
    return run.main(argv, extra_config=extra), seen


def test_run_cli_sub(tmp_path, monkeypatch):
    """`python -m clip_glass_amd.run --latent-space sub --subspace-components 8 --subspace-layers 0-3,4-7`: two NSGA-II generations on
    mini-sized synthetic weights, sized as tests/test_gpu_engine.py::test_run_cli_end_to_end sizes its run; then the same search from the
    basis file the first run wrote."""
    first = str(tmp_path / "probe")
    res, seen = _run_cli(first, monkeypatch)
    assert np.atleast_2d(res.X).shape[1] == 16 and np.atleast_2d(res.F).shape[1] == 2
    for f in ("genetic-it-1.jpg", "genetic-it-final.jpg", "genetic_result", "ls_result", "output.jpg", "subspace.npz"):
        assert os.path.getsize(os.path.join(first, f)) > 0, f
    saved = np.load(os.path.join(first, "ls_result"))
    assert list(saved.keys()) == ["sub", "w_plus"] and saved["sub"].shape == (8, 16) and saved["w_plus"].shape == (8, 8 * 32)
    assert set(pickle.load(open(os.path.join(first, "genetic_result"), "rb"))) == {"X", "F", "G", "CV"}
    X1, F1 = seen[0]
    assert X1.shape[1] == 16 and np.isfinite(F1).all() and len(set(F1[:, 0].tolist())) > 1
    basis = subspace.load(os.path.join(first, "subspace.npz"), latent_size=32)
    assert basis["components"].shape == (8, 32) and (np.diff(basis["stdev"]) <= 0).all()
    np.testing.assert_array_equal(basis["layer_group"], [0, 0, 0, 0, 1, 1, 1, 1])
    # layers 0-3 of a saved w+ row share group 0's step from the mean dlatent, layers 4-7 group 1's
    wp = saved["w_plus"].reshape(8, 8, 32)
    np.testing.assert_array_equal(wp[:, 0], wp[:, 3])
    np.testing.assert_array_equal(wp[:, 4], wp[:, 7])
    assert not np.array_equal(wp[:, 0], wp[:, 4])
    # the same seed from the written basis: the same search, bit for bit
    second = str(tmp_path / "file")
    res2, seen2 = _run_cli(second, monkeypatch, "--subspace-basis", os.path.join(first, "subspace.npz"))
    np.testing.assert_array_equal(np.atleast_2d(res2.X), np.atleast_2d(res.X))
    np.testing.assert_array_equal(np.atleast_2d(res2.F), np.atleast_2d(res.F))
    assert len(seen2) == len(seen) and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(seen, seen2))


def test_run_cli_sub_edit_latent(tmp_path, monkeypatch):
    """--edit-latent with a w+ row: the row is the subspace's base, the source picture is the zero row's, the search starts there."""
    from PIL import Image
    net_rows = synth.normal(21, "edit_w_plus", (8, 32), 1.0).astype(F32)
    row_file = str(tmp_path / "source_w_plus.npy")
    np.save(row_file, net_rows.reshape(-1))
    out = str(tmp_path / "edit")
    src_text = np.random.default_rng(12).standard_normal(32).astype(F32)
    from clip_glass_amd import run
    made = []
    inner = run.GenerationProblem.__init__

    def keep(self, *a, **k):
        inner(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(run.GenerationProblem, "__init__", keep)
    res, seen = _run_cli(out, monkeypatch, "--edit-latent", row_file, "--source-text", "a face", "--anchor-lambda", "0.5", config="StyleGAN2_ffhq_nod",
                         n_obj=1, source_text_features=src_text)
    gen = made[0].generator
    assert gen.latent_space == "sub" and not gen.edit_row.any() and gen.edit_row.shape == (16,)
    np.testing.assert_array_equal(gen.subspace["base"], net_rows)
    zero = np.zeros((4, 16), F32)
    np.testing.assert_array_equal(gen.engine.expand_latents(zero)[0], net_rows)          # the zero row IS the source
    np.testing.assert_array_equal(gen.source_image, gen.engine.generate(zero, generation=0, first_minibatch=0)[0])
    assert os.path.getsize(os.path.join(out, "source.jpg")) > 0
    assert Image.open(os.path.join(out, "source.jpg")).size == (32, 32)      # (written from gen.source_image by run.py)
    X1, _ = seen[0]
    assert not X1[0].any() and X1[1:].any()            # generation 0: the source itself, then steps of edit_sigma around it
    bad = str(tmp_path / "bad.npy")
    np.save(bad, np.zeros(33, F32))
    with pytest.raises(ValueError, match=r"a w row \(32 floats\) or a w\+ row \(256 floats\)"):
        _run_cli(str(tmp_path / "bad"), monkeypatch, "--edit-latent", bad, "--source-text", "a face", "--anchor-lambda", "0.5",
                 config="StyleGAN2_ffhq_nod", n_obj=1, source_text_features=src_text)


# ---- 9. feature off ----------------------------------------------------------------------------------------------------------------------
def test_default_engine_is_untouched(nets):
    """A z engine that never names the space launches what it launched before: the profile rows of the pass, no dlatents row at all, and
    the outputs of the same engine built with the setters at their defaults."""
    net = nets["mini"]
    z = synth.latents(1, 8, 32).astype(F32)
    outs, profs = [], []
    for explicit in (False, True):
        e = _engine("mini", net["sd"], net["avg"], finalize=False)
        if explicit:
            e.set_latent_space("z")
        e.finalize()
        e.set_target(net["target"])
        outs.append(_all_outputs(e, z, net["planes"]))
        e.set_profiling(1)
        e.evaluate(z, noise=net["planes"])
        profs.append([(r["name"], r["launches"]) for r in e.profile()])
        e.close()
    _same(outs[0], outs[1])
    assert profs[0] == profs[1]
    names = [n for n, _ in profs[0]]
    assert not [n for n in names if n.startswith("dlatents")] and [n for n in names if n.startswith("styles")] == ["styles"]
    assert dict(profs[0])["mapping"] == 1
    # and a sub engine adds exactly its own row in front of the truncation's
    sp = _space("mini", 6, "two_frozen_ends")
    e = _sub_engine("mini", net, sp, truncation_psi=0.5, truncation_cutoff=3)
    e.set_target(net["target"])
    e.set_profiling(1)
    e.evaluate(sp["rows"], noise=net["planes"])
    rows = [(r["name"], r["launches"]) for r in e.profile()]
    e.close()
    names = [n for n, _ in rows]
    assert "mapping" not in names and dict(rows)["dlatents.sub"] == 1 and dict(rows)["dlatents"] == 1 and dict(rows)["styles"] == 1
