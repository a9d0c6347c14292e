"""BigGAN-deep path (config C3) through the drop-in C ABI vs the oracle restatement
(oracle/biggan_ref.py — parity unpinned: pytorch-pretrained-biggan's source is absent, see its header).
Tolerance on CLIP similarity: 1e-3 relative (BASELINE.json north_star)."""
import numpy as np
import pytest
import torch

from clip_glass_amd import synth
from oracle import fitness_ref
import glass_models as M
from util import check, diag

pytestmark = pytest.mark.gpu


def _t(sd):
    return {k: torch.as_tensor(v) for k, v in sd.items()}


def _run_case(name, P, batch_size, chunk=0, seed=0, truncation=1.0):
    c = M.BIGGAN_CONFIGS[name]
    sd = M.make_biggan_state(name, seed)
    x = synth.biggan_population(seed + 1, P, c["z_dim"], c["num_classes"])
    x[0, :c["z_dim"]] *= 3.0   # exercise the clip to [-2, 2] (latent.py:21)
    detail = {}
    kw = dict(attention_pos=c["attention_pos"], ch=c["ch"])
    fitness_ref.evaluate_biggan(_t(sd), x, np.ones(c["clip"][5], np.float32), c["z_dim"], batch_size, truncation,
                                c["layers"], clip_size=c["clip"][4], detail=detail, **kw)
    feats = detail["features"].numpy()
    target = M.make_target(feats)
    sim_o = torch.cosine_similarity(detail["features"], torch.tensor(target)[None]).numpy()
    e = M.make_biggan_engine(name, sd, batch_size=batch_size, max_pop=P, chunk=chunk, truncation=truncation)
    e.set_target(target)
    Fe = e.evaluate(x)
    det = e.details(P)
    img = e.generate(x)
    e.close()
    tag = "%s P%d bs%d ch%d" % (name, P, batch_size, chunk)
    ref_img = detail["image"].numpy()
    rms = float(np.sqrt(((img - ref_img) ** 2).mean()))
    diag("[biggan] %s image rms err %.3e max %.3e" % (tag, rms, np.abs(img - ref_img).max()))
    assert rms < 2e-3, "image rms error %.3e" % rms
    check(tag + " clip features", det["features"], feats, 5e-3)
    rel = np.abs(det["sim"] - sim_o) / np.abs(sim_o)
    diag("[biggan] %s sim range [%.3f, %.3f] max rel err %.3e" % (tag, sim_o.min(), sim_o.max(), rel.max()))
    assert rel.max() < 1e-3, "CLIP similarity relative error %.3e > 1e-3" % rel.max()
    np.testing.assert_allclose(Fe[:, 0], -det["sim"], rtol=0, atol=1e-7)
    assert Fe.shape == (P, 1)
    return Fe


def test_biggan_mini_matches_oracle():
    _run_case("bg_mini", 8, 4)


def test_biggan_mini_chunking_invariant():
    a = _run_case("bg_mini", 8, 4, chunk=4)
    b = _run_case("bg_mini", 8, 8, chunk=8)
    np.testing.assert_array_equal(a, b)   # candidates are independent: minibatch / chunk are not semantic


def test_biggan_truncation_blend():
    _run_case("bg_mini", 4, 4, truncation=0.41)


def test_biggan_256_two_candidates():
    _run_case("bg256", 2, 2)


def test_biggan_512_two_candidates():
    _run_case("bg512", 2, 2)


def test_biggan_512_full_population():
    """BASELINE.json configs[2] at its real size: biggan-deep-512, pop = 64, batch_size = 8 (config.py:66) in ONE engine call —
    the launch sizes bench.py's `biggan512` leg times.  BigGAN candidates are independent (no minibatch statistics at inference),
    so the oracle scores 16 of the 64 rows (the first and the last minibatch: 2 x ~25 s of CPU instead of 8 x) and those rows of the
    64-row launch must meet it: image, CLIP features, similarity within 1e-3 relative."""
    name, P, bs = "bg512", 64, 8
    c = M.BIGGAN_CONFIGS[name]
    sd = M.make_biggan_state(name, 0)
    x = synth.biggan_population(11, P, c["z_dim"], c["num_classes"])
    rows = np.r_[0:8, 56:64]
    detail = {}
    fitness_ref.evaluate_biggan(_t(sd), x[rows], np.ones(c["clip"][5], np.float32), c["z_dim"], bs, 1.0, c["layers"],
                                clip_size=c["clip"][4], detail=detail, attention_pos=c["attention_pos"], ch=c["ch"])
    feats = detail["features"].numpy()
    target = M.make_target(feats)
    sim_o = torch.cosine_similarity(detail["features"], torch.tensor(target)[None]).numpy()
    e = M.make_biggan_engine(name, sd, batch_size=bs, max_pop=P)
    e.set_target(target)
    Fe = e.evaluate(x)
    det = e.details(P)
    img = e.generate(x)
    # the same rows scored as their own 8-row launches: rows do not depend on the launch they ride in
    F_first, F_last = e.evaluate(x[:8]), e.evaluate(x[56:])
    e.close()
    assert Fe.shape == (P, 1) and np.isfinite(Fe).all()
    ref_img = detail["image"].numpy()
    rms = float(np.sqrt(((img[rows] - ref_img) ** 2).mean()))
    rel = np.abs(det["sim"][rows] - sim_o) / np.abs(sim_o)
    diag("[biggan] bg512 P=64 bs=8 one launch, rows 0-7 + 56-63 vs oracle: image rms err %.3e max %.3e; sim range [%.3f, %.3f] max rel err %.3e"
         % (rms, np.abs(img[rows] - ref_img).max(), sim_o.min(), sim_o.max(), rel.max()))
    assert rms < 2e-3, "image rms error %.3e" % rms
    check("bg512 P=64 clip features", det["features"][rows], feats, 5e-3)
    assert rel.max() < 1e-3, "CLIP similarity relative error %.3e > 1e-3" % rel.max()
    np.testing.assert_allclose(Fe[:, 0], -det["sim"], rtol=0, atol=1e-7)
    d_launch = float(np.abs(np.concatenate([F_first, F_last]) - Fe[rows]).max())
    diag("[biggan] bg512 rows 0-7 / 56-63 as their own 8-row launches vs inside the 64-row launch: max |dF| %.3e" % d_launch)
    assert d_launch <= 1e-5      # (same kernel instances at every launch size: expected 0)


def test_biggan_512_eight_candidates_streaming_kernels():
    """P = 8 makes the 512^2 layers large enough (>= 4096 tiles) for conv_stream (the fused bn shift + relu epilogue of conv_2; the
    streaming kernel refuses in_up, so conv_1's nearest-up input addressing stays on conv_tiled), which the two-candidate case leaves
    to conv_tiled."""
    _run_case("bg512", 8, 8)


@pytest.mark.parametrize("name", ["bg_mini", "bg512"])
def test_biggan_per_block_taps(name):
    """Every GenBlock output and the self-attention output of the engine against the oracle's taps (biggan_ref.generator(taps=)):
    the path is parity-unpinned (package source absent), so a mismatch with a real checkpoint must be localisable to the first
    wrong block."""
    from oracle import biggan_ref
    c = M.BIGGAN_CONFIGS[name]
    P = 2
    sd = M.make_biggan_state(name, 0)
    x = synth.biggan_population(3, P, c["z_dim"], c["num_classes"])
    z, probs = biggan_ref.latent_forward(x, c["z_dim"])                            # latent.py:16-24
    taps = {}
    with torch.no_grad():
        biggan_ref.generator(_t(sd), z, probs, 1.0, c["layers"], attention_pos=c["attention_pos"], ch=c["ch"], taps=taps)
    e = M.make_biggan_engine(name, sd, batch_size=P, max_pop=P)
    worst = 0.0
    for key in ["block%d" % i for i in range(len(c["layers"]))] + ["attn"]:
        e.biggan_tap(-1 if key == "attn" else int(key[5:]))
        e.generate(x)
        got = e.biggan_tap_result().transpose(0, 3, 1, 2)                          # NHWC -> NCHW
        ref = taps[key].numpy()
        assert got.shape == ref.shape, (key, got.shape, ref.shape)
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        worst = max(worst, err)
        assert err < 1e-2, "%s: first wrong block is %s (max err %.3e of max |ref|)" % (name, key, err)
    diag("[biggan] %s per-block taps: %d blocks + attention, worst max-err / max|ref| = %.3e" % (name, len(c["layers"]), worst))
    e.close()


def test_biggan_fused_last_stage_matches_the_three_launch_path():
    """bg_tail.hip (conv_3 + skip -> bn -> relu -> conv_to_rgb -> tanh in one kernel, the 3x3 as a sum of MFMA partial products) against
    the three-launch path it replaces, on the SAME engine and inputs at biggan-deep-512 size: a tap request for the last block's output
    keeps that pass on the unfused kernels (biggan.cpp).  The two differ in where the 128-channel map is rounded to fp16 only."""
    name = "bg512"
    c = M.BIGGAN_CONFIGS[name]
    P = 2
    sd = M.make_biggan_state(name, 0)
    x = synth.biggan_population(5, P, c["z_dim"], c["num_classes"])
    e = M.make_biggan_engine(name, sd, batch_size=P, max_pop=P)
    fused = np.array(e.generate(x), np.float32)
    e.biggan_tap(len(c["layers"]) - 1)
    unfused = np.array(e.generate(x), np.float32)
    assert e.biggan_tap_result().shape[-1] == c["ch"]          # (the tap was taken: that pass ran conv_3 on its own)
    again = np.array(e.generate(x), np.float32)                 # one-shot tap: this pass is fused again, and deterministic
    e.close()
    np.testing.assert_array_equal(fused, again)
    err = float(np.abs(fused - unfused).max())
    diag("[biggan] fused last stage vs three launches at %s: max |diff| = %.3e (images in (-1, 1))" % (name, err))
    assert err < 4e-3


def test_biggan_error_paths():
    from clip_glass_amd.engine import Engine
    c = M.BIGGAN_CONFIGS["bg_mini"]
    with pytest.raises(RuntimeError, match="channel-drop"):
        Engine([], batch_size=4, max_pop=4, clip=c["clip"],
               biggan=dict(layers=[(0, 16, 16), (1, 16, 4), (1, 4, 1)], attention_pos=-1, ch=64, z_dim=16, num_classes=24))
    e = Engine([], batch_size=4, max_pop=4, clip=c["clip"],
               biggan=dict(layers=c["layers"], attention_pos=c["attention_pos"], ch=c["ch"], z_dim=16, num_classes=24))
    with pytest.raises(RuntimeError, match="missing tensor"):
        e.finalize()
    e.close()


def test_biggan_generation_problem_and_cli(tmp_path):
    """The reference-facing surface for the DeepMindBigGAN configs (run.py's default): GenerationProblem._evaluate on
    mixed [z | class bits] rows, then the CLI mirror with the native mixed-variable GA (pymoo absent)."""
    import os, pickle, types
    from clip_glass_amd import config as gconfig, run
    from clip_glass_amd.problem import GenerationProblem
    c = M.BIGGAN_CONFIGS["bg_mini"]
    sd = M.make_biggan_state("bg_mini", 0)
    x = synth.biggan_population(4, 8, c["z_dim"], c["num_classes"])
    kw = dict(attention_pos=c["attention_pos"], ch=c["ch"])
    detail = {}
    fitness_ref.evaluate_biggan(_t(sd), x, np.ones(c["clip"][5], np.float32), c["z_dim"], 4, 1.0, c["layers"],
                                clip_size=c["clip"][4], detail=detail, **kw)
    target = M.make_target(detail["features"].numpy())
    Fo, Go = fitness_ref.evaluate_biggan(_t(sd), x, target, c["z_dim"], 4, 1.0, c["layers"], clip_size=c["clip"][4], **kw)
    n_var = c["z_dim"] + c["num_classes"]
    extra = dict(weights="synthetic:0", clip_weights="synthetic:0", dim_z=c["z_dim"], num_classes=c["num_classes"],
                 biggan_geometry=dict(layers=c["layers"], attention_pos=c["attention_pos"], ch=c["ch"]),
                 clip_geometry=c["clip"], target_features=target, batch_size=4,
                 problem_args=dict(n_var=n_var, n_obj=1, n_constr=c["z_dim"], xl=-2, xu=2))
    cfg = types.SimpleNamespace(config="DeepMindBigGAN512", device="cuda", target="unused")
    vars(cfg).update(gconfig.get_config("DeepMindBigGAN512"))
    vars(cfg).update(extra)
    prob = GenerationProblem(cfg)
    out = {}
    prob._evaluate(x.astype(object), out)        # pymoo hands mixed-variable populations over as object arrays
    assert out["F"].shape == (8,) and out["F"].dtype == np.float32 and out["G"].shape == (8,)
    rel = np.abs(out["F"] - Fo) / np.abs(Fo)
    diag("[biggan] GenerationProblem drop-in: sim rel err %.3e" % rel.max())
    assert rel.max() < 1e-3
    ls = cfg.latent(cfg)
    ls.set_from_population(x[:3])
    img = prob.generator.generate(ls)
    assert img.shape == (3, 3, 64, 64) and img.min() >= 0 and img.max() <= 1
    prob.generator.engine.close()
    argv = ["--config", "DeepMindBigGAN512", "--generations", "3", "--save-each", "2", "--tmp-folder", str(tmp_path),
            "--pop-size", "8"]
    res = run.main(argv, extra_config=extra)
    for f in ("genetic-it-2.jpg", "genetic-it-final.jpg", "genetic_result", "ls_result", "output.jpg"):
        assert os.path.getsize(os.path.join(str(tmp_path), f)) > 0, f
    d = pickle.load(open(os.path.join(str(tmp_path), "genetic_result"), "rb"))
    assert np.atleast_2d(d["X"]).shape[1] == n_var
