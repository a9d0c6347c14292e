"""Latent spaces (z / w / w+) and the truncation trick through the C ABI, on the GPU: map_latents against a float64 restatement, every
mode against the reference's own Generator (tests/golden/dlatent_modules.npz) and the oracle helper (tests/dlatent_ref.py), the bitwise
identities between the spaces, psi = 0, slices and chunks, the refusals, and one run.py search in w+."""
import math
import os
import pickle

import numpy as np
import pytest
import torch

import dlatent_ref as R
import glass_models as M
from clip_glass_amd import synth
from clip_glass_amd.engine import Engine
from oracle import stylegan2_ref as sg
from util import check, check_logits, diag

pytestmark = pytest.mark.gpu
MODES = [("z", 0.7, None), ("z", 0.5, 3), ("w", 1.0, None), ("w+", 1.0, None), ("w+", 0.5, 3)]


def _t(sd):
    return {k: torch.as_tensor(v) for k, v in sd.items()}


def _engine(name, sd, avg=None, *, P=8, use_d=True, noise_mode=2, noise_seed=0, chunk=0, finalize=True, **latent):
    c = M.CONFIGS[name]
    e = Engine(c["channels"][::-1], latent_size=c["latent"], mapping_layers=c["mapping"], batch_size=4, use_discriminator=use_d,
               n_obj=2 if use_d else 1, max_pop=P, chunk=chunk, clip=c["clip"], noise_mode=noise_mode, noise_seed=noise_seed, **latent)
    e.load_state(sd)
    if avg is not None:
        e.load_tensor("dlatent_avg", avg)
    if finalize:
        e.finalize()
    return e


def _oracle_map(tsd, z):
    with torch.no_grad():
        return sg.g_mapping(tsd, torch.tensor(np.asarray(z, np.float32))).numpy()


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(R.FIXTURE))


@pytest.fixture(scope="module")
def cases(fx):
    """Per network: weights, dlatent_avg, two minibatches of noise planes and the population of every space — P = 8, the first four rows
    of `mini` being the fixture's."""
    out = {}
    for name, seed in (("mini", R.SEED), ("mid", 0)):
        c = M.CONFIGS[name]
        sd = M.make_state(name, seed)
        L, n_lat = c["latent"], 2 * len(c["channels"])
        if name == "mini":
            planes = [synth.g_noise_planes(7, 0, m, c["channels"]) for m in range(2)]
            z = np.concatenate([fx["z"], synth.latents(2, 4, L).astype(np.float32)])
        else:
            planes = M.noise_planes(name, 77, 3, 2)
            z = synth.latents(1, 8, L).astype(np.float32)
        tsd = _t(sd)
        w = _oracle_map(tsd, z)
        wp = (w[:, None, :] + synth.normal(12, "w_plus8", (8, n_lat, L), 0.3)).astype(np.float32)
        if name == "mini":
            w[:4], wp[:4] = fx["w"], fx["w_plus"]
        out[name] = dict(sd=sd, tsd=tsd, avg=synth.dlatent_avg(L, seed), planes=planes, n_lat=n_lat,
                         rows={"z": z, "w": w, "w+": wp.reshape(8, -1)})
    return out


# ---- 1. map_latents ------------------------------------------------------------------------------------------
def _map64(sd, z):
    """float64 restatement of stylegan2/models.py:590-627: pixel norm, then dense (coef lr_mul / sqrt(L)) + bias * lr_mul + lrelu * sqrt2."""
    x = np.asarray(z, np.float64)
    x = x / np.sqrt((x ** 2).mean(axis=1, keepdims=True) + 1e-8)
    i = 0
    while "G_mapping.main.%d.layer.weight" % i in sd:
        W = np.asarray(sd["G_mapping.main.%d.layer.weight" % i], np.float64)
        b = np.asarray(sd["G_mapping.main.%d.bias" % i], np.float64)
        x = x @ (W * (0.01 / math.sqrt(W.shape[1]))).T + b * 0.01
        x = np.where(x >= 0, x, 0.2 * x) * math.sqrt(2.0)
        i += 1
    return x


@pytest.mark.parametrize("L,layers,P", [(32, 2, 8), (512, 8, 8), (32, 2, 5), (512, 8, 5)])
def test_map_latents_matches_float64(L, layers, P):
    """Bar: 4 x the error of oracle.g_mapping (torch fp32 on the CPU) against the same float64 values on these inputs — the kernel's
    16-way split sums in another order than torch does.  L = 32 runs the per-layer path, L = 512 mapping_fused_kernel<2>; P = 5 leaves
    the tail of a 4-candidate workgroup.
    Measured on an MI355X, max abs error against float64 (max |w| 4.5 at L = 32, 7.4 / 6.7 at L = 512), oracle fp32 / engine:
    L = 32 x 2, P = 8: 9.5e-7 / 1.07e-6; P = 5: 9.5e-7 / 9.5e-7.  L = 512 x 8, P = 8: 5.97e-6 / 3.82e-6; P = 5: 5.88e-6 / 3.82e-6.
    Against the reference's own G_mapping (fixture, next test): 9.5e-7 under a bar of 3.6e-6."""
    ch = [16, 16, 32, 32]
    clip = M.CONFIGS["mini"]["clip"]
    sd = synth.make_state(synth.stylegan2_g_spec(ch, L, layers), 4)
    sd.update(synth.make_state(synth.clip_visual_spec(clip[0], clip[1], clip[3], clip[4], clip[5]), 4))
    z = synth.latents(9, P, L).astype(np.float32)
    ref = _map64(sd, z)
    err_o = float(np.abs(_oracle_map(_t(sd), z) - ref).max())
    e = Engine(ch[::-1], latent_size=L, mapping_layers=layers, batch_size=4, use_discriminator=False, n_obj=1, max_pop=8, clip=clip,
               noise_mode=0)
    e.load_state(sd)
    e.finalize()
    w = e.map_latents(z)
    e.close()
    err_e = float(np.abs(w - ref).max())
    diag("[dlatents] map_latents L%d x%d P%d: max|ref| %.3f oracle fp32 err %.3e engine err %.3e bar %.3e" % (L, layers, P, np.abs(ref).max(), err_o, err_e, 4 * err_o))
    assert w.shape == (P, L) and w.dtype == np.float32
    assert err_e <= 4 * err_o


def test_map_latents_matches_the_reference_fixture(fx, cases):
    c = cases["mini"]
    z = c["rows"]["z"]
    bar = 4 * float(np.abs(_oracle_map(c["tsd"], z) - _map64(c["sd"], z)).max())
    e = _engine("mini", c["sd"], use_d=False)
    w = e.map_latents(z)
    e.close()
    err = float(np.abs(w[:4] - fx["w"]).max())
    diag("[dlatents] map_latents vs the reference's G_mapping: err %.3e bar %.3e" % (err, bar))
    assert err <= bar


# ---- 2. parity of every mode -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mini", "mid"])
@pytest.mark.parametrize("space,psi,cutoff", MODES)
def test_mode_matches_oracle_and_reference(cases, fx, name, space, psi, cutoff):
    """The bars of tests/test_gpu_engine.py::_run_case, against tests/dlatent_ref.py; on `mini` the first minibatch's images also against
    what the reference's Generator produced."""
    c, cfg = cases[name], M.CONFIGS[name]
    x, planes = c["rows"][space], c["planes"]
    mode = dict(space=space, psi=psi, cutoff=cutoff, avg=c["avg"])
    detail = {}
    R.evaluate(c["tsd"], x, np.ones(cfg["clip"][5], np.float32), 4, True, lambda i: planes[i], clip_size=cfg["clip"][4], detail=detail, **mode)
    feats = detail["features"].numpy()
    target = M.make_target(feats)
    sim_o = torch.cosine_similarity(detail["features"], torch.tensor(target)[None]).numpy()
    e = _engine(name, c["sd"], c["avg"], latent_space=space, truncation_psi=psi, truncation_cutoff=cutoff)
    assert e.latent_row() == (x.shape[1], c["n_lat"])
    e.set_target(target)
    Fe = e.evaluate(x, noise=planes)
    det = e.details(8)
    img = e.generate(x, noise=planes)
    e.close()
    tag = "%s %s psi%.1f cut%s" % (name, space, psi, cutoff)
    ref_img = detail["image"].numpy()
    rms = float(np.sqrt(((img - ref_img) ** 2).mean()))
    diag("[dlatents] %s image rms err %.3e" % (tag, rms))
    assert rms < 1e-3, "image rms error %.3e" % rms
    check(tag + " image", img, ref_img, 3e-2)
    check(tag + " clip features", det["features"], feats, 5e-3)
    rel = np.abs(det["sim"] - sim_o) / np.abs(sim_o)
    diag("[dlatents] %s sim range [%.3f, %.3f] max rel err %.3e" % (tag, sim_o.min(), sim_o.max(), rel.max()))
    assert rel.max() < 1e-3, "CLIP similarity relative error %.3e > 1e-3" % rel.max()
    np.testing.assert_allclose(Fe[:, 0], -det["sim"], rtol=0, atol=1e-7)
    dis_o = detail["dis"].numpy()[:, 0]
    check_logits(tag + " D logits", det["dis"], dis_o, case=name)
    check_logits(tag + " hinge", Fe[:, 1], np.maximum(1 - dis_o, 0), case=name)
    if name == "mini":
        key = {("z", 0.7): "img_z_psi07", ("z", 0.5): "img_z_psi05_cut3", ("w", 1.0): "img_w", ("w+", 1.0): "img_w_plus",
               ("w+", 0.5): "img_w_plus_psi05_cut3"}[(space, psi)]
        fix = np.clip((fx[key] + 1) / 2.0, 0, 1)             # utils.py:14-17 biggan_norm
        rms = float(np.sqrt(((img[:4] - fix) ** 2).mean()))
        diag("[dlatents] %s vs the reference's Generator: image rms err %.3e" % (tag, rms))
        assert rms < 1e-3
        check(tag + " image vs reference", img[:4], fix, 3e-2)


# ---- 3. bitwise identities ---------------------------------------------------------------------------------------
def _all_outputs(e, x, planes):
    F = e.evaluate(x, noise=planes)
    det = e.details(x.shape[0])
    return dict(F=F, features=det["features"], dis=det["dis"], img=e.generate(x, noise=planes))


def _same(a, b):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.fixture(scope="module")
def z_pass(cases):
    """The default engine's pass over z, its mapped rows, and its profile: the left-hand side of the identities below."""
    c = cases["mini"]
    e = _engine("mini", c["sd"], c["avg"])
    e.set_target(M.make_target(np.ones((8, 32), np.float32), seed=3))
    z = c["rows"]["z"]
    out = _all_outputs(e, z, c["planes"])
    w = e.map_latents(z)
    e.set_truncation(1.0, 3)               # psi = 1 with a cutoff: still off
    out_psi1 = _all_outputs(e, z, c["planes"])
    e.set_truncation(1.0, None)
    e.set_profiling(1)
    e.evaluate(z, noise=c["planes"])
    prof = [(r["name"], r["launches"]) for r in e.profile()]
    e.close()
    return dict(out=out, w=w, out_psi1=out_psi1, prof=prof, target=M.make_target(np.ones((8, 32), np.float32), seed=3))


def test_w_and_w_plus_on_mapped_rows_equal_z(cases, z_pass):
    c = cases["mini"]
    assert np.isfinite(z_pass["out"]["F"]).all() and len(set(z_pass["out"]["F"][:, 0])) > 1
    for space, rows in (("w", z_pass["w"]), ("w+", np.tile(z_pass["w"], (1, c["n_lat"])))):
        e = _engine("mini", c["sd"], c["avg"], latent_space=space)
        e.set_target(z_pass["target"])
        _same(z_pass["out"], _all_outputs(e, rows, c["planes"]))
        e.close()


def test_psi_one_with_any_cutoff_is_psi_never_set(z_pass):
    _same(z_pass["out"], z_pass["out_psi1"])


def test_setters_at_their_defaults_change_nothing(cases, z_pass):
    c = cases["mini"]
    e = _engine("mini", c["sd"], c["avg"], finalize=False)
    e.set_latent_space("z")
    e.set_truncation(1.0, None)
    e.finalize()
    e.set_target(z_pass["target"])
    _same(z_pass["out"], _all_outputs(e, c["rows"]["z"], c["planes"]))
    e.set_profiling(1)
    e.evaluate(c["rows"]["z"], noise=c["planes"])
    prof = [(r["name"], r["launches"]) for r in e.profile()]
    e.close()
    assert prof == z_pass["prof"]
    assert not [n for n, _ in prof if n.startswith("dlatents")] and [n for n, _ in prof if n.startswith("styles")] == ["styles"]


def test_profile_rows_of_the_layered_path(cases):
    c = cases["mini"]
    e = _engine("mini", c["sd"], c["avg"], latent_space="z", truncation_psi=0.5, truncation_cutoff=3)
    e.set_target(np.ones(32, np.float32))
    e.set_profiling(1)
    e.evaluate(c["rows"]["z"], noise=c["planes"])
    rows = {r["name"]: r for r in e.profile()}
    e.close()
    assert rows["dlatents"]["launches"] == 1 and rows["styles"]["launches"] == 1 and rows["mapping"]["launches"] == 1
    assert rows["dlatents"]["bytes"] == 4 * 32 * (8 * (8 + 1) + 1)          # reads P rows + avg, writes P n_lat rows


# ---- 4. psi = 0 ----------------------------------------------------------------------------------------------------
def test_psi_zero_is_the_average_dlatent(cases):
    c = cases["mini"]
    e = _engine("mini", c["sd"], c["avg"], use_d=False, truncation_psi=0.0)
    img = e.generate(c["rows"]["z"], noise=c["planes"])
    e.close()
    for m in range(2):                      # one noise plane per minibatch: its four images are one image
        for i in range(1, 4):
            np.testing.assert_array_equal(img[4 * m + i], img[4 * m])
    assert not np.array_equal(img[0], img[4])
    e = _engine("mini", c["sd"], c["avg"], use_d=False, latent_space="w")
    img_w = e.generate(np.tile(c["avg"], (8, 1)), noise=c["planes"])
    e.close()
    np.testing.assert_array_equal(img, img_w)


# ---- 5. slices and chunks in w+ -----------------------------------------------------------------------------------
def test_w_plus_chunks_and_slices(cases):
    c = cases["mini"]
    rows = np.concatenate([c["rows"]["w+"], c["rows"]["w+"][::-1] * np.float32(0.9)])         # P = 16
    Fs = []
    for chunk in (4, 16):
        e = _engine("mini", c["sd"], c["avg"], P=16, noise_mode=1, noise_seed=77, chunk=chunk, latent_space="w+", truncation_psi=0.5,
                    truncation_cutoff=3)
        e.set_target(M.make_target(np.ones((8, 32), np.float32), seed=3))
        Fs.append(e.evaluate(rows, generation=2))
        if chunk == 16:
            whole = e.evaluate(rows[:8], generation=2)
            parts = [e.evaluate(rows[4 * m:4 * m + 4], generation=2, first_minibatch=m) for m in range(2)]
            np.testing.assert_array_equal(np.concatenate(parts), whole)
            np.testing.assert_array_equal(whole, Fs[-1][:8])
        e.close()
    assert np.isfinite(Fs[0]).all() and len(set(Fs[0][:, 0])) > 1
    np.testing.assert_array_equal(Fs[0], Fs[1])


# ---- 6. refusals -----------------------------------------------------------------------------------------------------
def test_refusals(cases):
    c = cases["mini"]
    e = _engine("mini", c["sd"], c["avg"], latent_space="w+")
    e.set_target(np.ones(32, np.float32))
    for bad in (c["rows"]["z"], c["rows"]["w+"][:, :-1], c["rows"]["w+"][0]):
        with pytest.raises(ValueError, match=r"\[P, 256\]"):
            e.evaluate(bad, noise=c["planes"])                 # refused in Python: the library never sees the short rows
        with pytest.raises(ValueError, match=r"\[P, 256\]"):
            e.generate(bad, noise=c["planes"])
    with pytest.raises(RuntimeError, match="finalized"):
        e.set_latent_space("z")
    with pytest.raises(RuntimeError, match="max_pop"):
        e.map_latents(np.zeros((9, 32), np.float32))
    with pytest.raises(ValueError, match=r"\[P, 32\]"):
        e.map_latents(np.zeros((4, 256), np.float32))
    for psi, msg in ((-0.5, "psi < 0"), (1.5, "psi > 1"), (float("nan"), "finite")):
        with pytest.raises(RuntimeError, match=msg):
            e.set_truncation(psi)
    with pytest.raises(RuntimeError, match="cutoff"):
        e.set_truncation(0.5, 9)
    e.set_truncation(0.5, 8)                                   # cutoff = n_lat is every layer
    e.close()
    # psi != 1 without dlatent_avg: at finalize when the setter came first, in the setter after it
    e = _engine("mini", c["sd"], None, finalize=False, truncation_psi=0.7)
    with pytest.raises(RuntimeError, match="dlatent_avg"):
        e.finalize()
    e.close()
    e = _engine("mini", c["sd"], None)
    with pytest.raises(RuntimeError, match="dlatent_avg"):
        e.set_truncation(0.7)
    e.set_truncation(1.0, 3)                                   # off: needs no average
    e.close()
    # a cutoff inside (0, n_lat) on an engine finalized without the per-layer buffer
    e = _engine("mini", c["sd"], c["avg"])
    e.set_truncation(0.7)                                      # every layer: one row per candidate
    with pytest.raises(RuntimeError, match="per-layer buffer"):
        e.set_truncation(0.7, 3)
    e.close()
    # BigGAN: no mapping network, no dlatents
    b = M.BIGGAN_CONFIGS["bg_mini"]
    geo = dict(layers=b["layers"], attention_pos=b["attention_pos"], ch=b["ch"], z_dim=b["z_dim"], num_classes=b["num_classes"])
    with pytest.raises(RuntimeError, match="StyleGAN2"):
        Engine([], batch_size=4, max_pop=8, clip=b["clip"], biggan=geo, latent_space="w")
    with pytest.raises(RuntimeError, match="StyleGAN2"):
        Engine([], batch_size=4, max_pop=8, clip=b["clip"], biggan=geo, truncation_psi=0.7)
    eb = Engine([], batch_size=4, max_pop=8, clip=b["clip"], biggan=geo)
    assert eb.latent_row() == (b["z_dim"] + b["num_classes"], 0)
    eb.close()


# ---- 7. run.py --------------------------------------------------------------------------------------------------------
def test_run_cli_w_plus_truncated(tmp_path, monkeypatch):
    """`python -m clip_glass_amd.run --latent-space w+ --truncation-psi 0.7`: two NSGA-II generations on mini-sized synthetic weights, sized
    as tests/test_gpu_engine.py::test_run_cli_end_to_end sizes its run."""
    from clip_glass_amd import run
    c = M.CONFIGS["mini"]
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "mini_problem.npz")))
    extra = dict(channels=c["channels"], dim_z=c["latent"], mapping_layers=c["mapping"], clip_geometry=c["clip"],
                 clip_text_geometry=dict(width=64, layers=2), target_features=g["text_features"],
                 problem_args=dict(n_var=c["latent"], n_obj=2, n_constr=c["latent"], xl=-10, xu=10))
    seen = []
    inner = run.GenerationProblem._evaluate

    def recording(self, x, out, *a, **k):
        inner(self, x, out, *a, **k)
        seen.append((np.array(x), np.array(out["F"])))
    monkeypatch.setattr(run.GenerationProblem, "_evaluate", recording)
    argv = ["--config", "StyleGAN2_ffhq_d", "--generations", "2", "--save-each", "1", "--tmp-folder", str(tmp_path), "--weights", "synthetic:0",
            "--clip-weights", "synthetic:0", "--pop-size", "8", "--latent-space", "w+", "--truncation-psi", "0.7"]
    res = run.main(argv, extra_config=extra)
    width = 8 * c["latent"]
    assert np.atleast_2d(res.X).shape[1] == width and np.atleast_2d(res.F).shape[1] == 2
    for f in ("genetic-it-1.jpg", "genetic-it-final.jpg", "genetic_result", "ls_result", "output.jpg"):
        assert os.path.getsize(os.path.join(str(tmp_path), f)) > 0, f
    saved = np.load(os.path.join(str(tmp_path), "ls_result"))
    assert list(saved.keys()) == ["w_plus"] and saved["w_plus"].shape[1] == width
    assert set(pickle.load(open(os.path.join(str(tmp_path), "genetic_result"), "rb"))) == {"X", "F", "G", "CV"}
    X1, F1 = seen[0]                       # generation 1: the mapped initial population, every layer the same dlatent
    assert X1.shape[1] == width and np.isfinite(F1).all() and len(set(F1[:, 0].tolist())) > 1
    np.testing.assert_array_equal(X1[:, :c["latent"]], X1[:, -c["latent"]:])
