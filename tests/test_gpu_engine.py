"""End-to-end parity through the drop-in C ABI (include/glass.h): engine.evaluate /
generate vs the oracle's `_evaluate` restatement on the same seeded weights, latents
and noise.  Tolerance on CLIP similarity: 1e-3 relative (BASELINE.json north_star)."""
import numpy as np
import pytest
import torch

from clip_glass_amd import synth
from oracle import fitness_ref
import glass_models as M
from util import check, check_logits, diag

pytestmark = pytest.mark.gpu


def _t(sd):
    return {k: torch.as_tensor(v) for k, v in sd.items()}


def _run_case(name, P, batch_size, use_d, noise_mode, chunk=0, seed=0):
    c = M.CONFIGS[name]
    sd = M.make_state(name, seed, with_d=use_d)
    x = synth.latents(seed + 1, P, c["latent"])
    n_mb = P // batch_size
    planes = M.noise_planes(name, 77, 3, n_mb)
    tsd = _t(sd)
    detail = {}
    noise_fn = (lambda i: planes[i]) if noise_mode else None
    # oracle pass 1 (features) -> target -> oracle F
    Fo, Go = fitness_ref.evaluate(tsd, x, np.ones(c["clip"][5], np.float32), batch_size, use_d, noise_fn,
                                  clip_size=c["clip"][4], detail=detail)
    feats = detail["features"].numpy()
    target = M.make_target(feats)
    sim_o = torch.cosine_similarity(detail["features"], torch.tensor(target)[None]).numpy()
    e = M.make_engine(name, sd, batch_size=batch_size, use_discriminator=use_d, max_pop=P,
                      noise_mode=noise_mode, noise_seed=77, chunk=chunk)
    e.set_target(target)
    Fe = e.evaluate(x, generation=3, noise=planes if noise_mode == 2 else None)
    det = e.details(P)
    img = e.generate(x, generation=3, noise=planes if noise_mode == 2 else None)
    e.close()
    tag = "%s P%d bs%d d%d nm%d ch%d" % (name, P, batch_size, use_d, noise_mode, chunk)
    ref_img = detail["image"].numpy()
    rms = float(np.sqrt(((img - ref_img) ** 2).mean()))
    diag("[e2e] %s image rms err %.3e" % (tag, rms))
    assert rms < 1e-3, "image rms error %.3e" % rms
    check(tag + " image", img, ref_img, 3e-2)   # fp16 activations: worst pixel of 12.6M, image range [0,1]
    check(tag + " clip features", det["features"], feats, 5e-3)
    rel = np.abs(det["sim"] - sim_o) / np.abs(sim_o)
    diag("[e2e] %s sim range [%.3f, %.3f] max rel err %.3e" % (tag, sim_o.min(), sim_o.max(), rel.max()))
    assert rel.max() < 1e-3, "CLIP similarity relative error %.3e > 1e-3" % rel.max()
    np.testing.assert_allclose(Fe[:, 0], -det["sim"], rtol=0, atol=1e-7)
    if use_d:
        dis_o = detail["dis"].numpy()[:, 0]
        check_logits(tag + " D logits", det["dis"], dis_o, case=name)
        check_logits(tag + " hinge", Fe[:, 1], np.maximum(1 - dis_o, 0), case=name)
    return Fe


@pytest.mark.parametrize("name", ["mini", "mid"])
@pytest.mark.parametrize("use_d", [True, False])
def test_evaluate_matches_oracle_explicit_noise(name, use_d):
    _run_case(name, P=8, batch_size=4, use_d=use_d, noise_mode=2)


def test_evaluate_device_noise_and_chunking():
    """Device Philox noise == numpy mirror fed to the oracle; result independent of chunk size."""
    F1 = _run_case("mini", P=16, batch_size=4, use_d=True, noise_mode=1, chunk=4)
    F2 = _run_case("mini", P=16, batch_size=4, use_d=True, noise_mode=1, chunk=16)
    np.testing.assert_array_equal(F1, F2)


def test_batch_size_semantics():
    """batch_size is semantic (noise sharing + mbstd groups): bs=8 groups != bs=4 groups, both match the oracle."""
    _run_case("mini", P=8, batch_size=8, use_d=True, noise_mode=2)


def test_no_noise():
    _run_case("mini", P=4, batch_size=4, use_d=True, noise_mode=0)


def test_error_paths():
    sd = M.make_state("mini", 0)
    e = M.make_engine("mini", sd, max_pop=8, noise_mode=0)
    x = synth.latents(1, 6, 32)
    with pytest.raises(RuntimeError, match="multiple of batch_size"):
        e.evaluate(x)            # reference: assert z.shape[0] % minibatch == 0 (models.py:112)
    with pytest.raises(RuntimeError, match="set_target"):
        e.evaluate(synth.latents(1, 8, 32))
    with pytest.raises(RuntimeError, match="max_pop"):
        e.generate(synth.latents(1, 12, 32))
    e.close()
    from clip_glass_amd.engine import Engine
    e2 = Engine([32, 32, 16, 16], latent_size=32, mapping_layers=2, clip=M.CONFIGS["mini"]["clip"])
    with pytest.raises(RuntimeError, match="missing tensor"):
        e2.finalize()            # reference: sys.exit(1) on missing weights (models.py:93-101)
    e2.close()


def test_full_size_ffhq_one_minibatch():
    """StyleGAN2 ffhq config-f 1024 px + D + CLIP ViT-B/32 at true sizes, P=4 (one minibatch)."""
    import time
    t = time.time()
    _run_case("ffhq", P=4, batch_size=4, use_d=True, noise_mode=2, chunk=4)
    diag("[e2e] full-size ffhq P=4 wall (oracle + engine + weight synthesis): %.1f s" % (time.time() - t))


def test_generation_problem_drop_in():
    """The reference-facing surface: config -> GenerationProblem(config)._evaluate(x, out) -> out["F"], out["G"]
    plus problem.generator.generate()/save() as run.py's callbacks use them (run.py:45-51,118-125)."""
    import types
    from clip_glass_amd import config as gconfig
    from clip_glass_amd.problem import GenerationProblem
    name = "mini"
    c = M.CONFIGS[name]
    sd = M.make_state(name, 0)
    tsd = _t(sd)
    x = synth.latents(1, 8, c["latent"])
    planes = [synth.g_noise_planes(42, 0, m, c["channels"]) for m in range(2)]
    detail = {}
    fitness_ref.evaluate(tsd, x, np.ones(c["clip"][5], np.float32), 4, True, lambda i: planes[i], clip_size=c["clip"][4], detail=detail)
    target = M.make_target(detail["features"].numpy())
    Fo, Go = fitness_ref.evaluate(tsd, x, target, 4, True, lambda i: planes[i], clip_size=c["clip"][4])
    cfg = types.SimpleNamespace(config="StyleGAN2_ffhq_d", device="cuda", target="unused")
    vars(cfg).update(gconfig.get_config("StyleGAN2_ffhq_d"))
    vars(cfg).update(weights="synthetic:0", clip_weights="synthetic:0", channels=c["channels"], dim_z=c["latent"],
                     mapping_layers=c["mapping"], clip_geometry=c["clip"], target_features=target, noise_mode=1,
                     noise_seed=42, problem_args=dict(cfg.problem_args, n_var=c["latent"], n_constr=c["latent"]))
    prob = GenerationProblem(cfg)
    out = {}
    prob._evaluate(x, out)
    assert out["F"].shape == (8, 2) and out["F"].dtype == np.float32 and out["G"].shape == (8,) and not out["G"].any()
    rel = np.abs(out["F"][:, 0] - Fo[:, 0]) / np.abs(Fo[:, 0])
    diag("[e2e] GenerationProblem drop-in: sim rel err %.3e, hinge abs err %.3e" % (rel.max(), np.abs(out["F"][:, 1] - Fo[:, 1]).max()))
    assert rel.max() < 1e-3
    check_logits("drop-in hinge", out["F"][:, 1], Fo[:, 1], case="mini")
    ls = cfg.latent(cfg)
    ls.set_from_population(x[:3])
    img = prob.generator.generate(ls)                      # run.py:118 — no minibatch argument
    assert img.shape == (3, 3, 32, 32) and img.min() >= 0 and img.max() <= 1
    import tempfile, os
    p = os.path.join(tempfile.mkdtemp(), "o.png")
    prob.generator.save(img, p)
    assert os.path.getsize(p) > 0
    prob.generator.engine.close()


def test_text_tower_matches_oracle_and_golden_tokens():
    """glass_engine_encode_text vs the oracle's CLIP.encode_text restatement (clip/model.py:307-320) on the
    token ids the reference tokenizer produced for the default target (tests/golden/mini_problem.npz)."""
    import os
    from oracle import clip_ref
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "mini_problem.npz")))
    tokens = np.stack([g["tokens"], np.r_[g["tokens"][:5], 49407, np.zeros(71, np.int64)]]).astype(np.int64)
    sd = M.make_state("mini", 0)
    sd.update(synth.make_state(synth.clip_text_spec(width=64, layers=2, out_dim=M.CONFIGS["mini"]["clip"][5]), 0))
    e = M.make_engine("mini", sd, max_pop=8, noise_mode=0)
    got = e.encode_text(tokens)
    e.close()
    ref = clip_ref.encode_text(_t(sd), torch.tensor(tokens)).numpy()
    check("text tower (mini)", got, ref, 3e-3)
    # the golden's text_features came from the REFERENCE's encode_text on the same weights / tokens
    check("text tower vs reference golden", got[0], g["text_features"], 3e-3)


def test_run_cli_end_to_end(tmp_path):
    """`python -m clip_glass_amd.run` mirror of run.py: a few NSGA-II generations on the mini architecture with a
    TEXT target (tokenizer + device text tower), periodic image dumps, result pickle, final output."""
    import os, pickle
    bpe = "/root/reference/assets/bpe_simple_vocab_16e6.txt.gz"
    from clip_glass_amd import run
    c = M.CONFIGS["mini"]
    extra = dict(channels=c["channels"], dim_z=c["latent"], mapping_layers=c["mapping"], clip_geometry=c["clip"],
                 clip_text_geometry=dict(width=64, layers=2), problem_args=dict(n_var=c["latent"], n_obj=2, n_constr=c["latent"], xl=-10, xu=10))
    if not os.path.exists(bpe):   # no vocab on the GPU box: use the text feature the reference produced (golden)
        g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "mini_problem.npz")))
        extra["target_features"] = g["text_features"]
    argv = ["--config", "StyleGAN2_ffhq_d", "--generations", "3", "--save-each", "2", "--tmp-folder", str(tmp_path),
            "--weights", "synthetic:0", "--clip-weights", "synthetic:0", "--pop-size", "8", "--bpe-path", bpe]
    res = run.main(argv, extra_config=extra)
    assert np.atleast_2d(res.F).shape[1] == 2
    for f in ("genetic-it-2.jpg", "genetic-it-final.jpg", "genetic_result", "ls_result", "output.jpg"):
        assert os.path.getsize(os.path.join(str(tmp_path), f)) > 0, f
    d = pickle.load(open(os.path.join(str(tmp_path), "genetic_result"), "rb"))
    assert set(d) == {"X", "F", "G", "CV"}


def test_offset_shards_equal_whole_population():
    """SURVEY 8(e) / config C4 on one GPU: a population evaluated as two contiguous shards with first_minibatch offsets
    (what ranks 0 and 1 of a 2-GPU job do, parallel.py) equals the single-call result — device noise is a pure function
    of (seed, generation, GLOBAL minibatch, layer) and mbstd groups never straddle a shard (models.py:108-129)."""
    from clip_glass_amd.parallel import shard_bounds
    name, P, bs = "mini", 16, 4
    c = M.CONFIGS[name]
    sd = M.make_state(name, 0)
    x = synth.latents(7, P, c["latent"])
    e = M.make_engine(name, sd, batch_size=bs, use_discriminator=True, max_pop=P, noise_mode=1, noise_seed=99)
    e.set_target(np.ones(c["clip"][5], np.float32))
    e.evaluate(x, generation=5)
    target = M.make_target(e.details(P)["features"])
    e.set_target(target)
    F_whole = e.evaluate(x, generation=5)
    for world in (2, 4):
        parts = []
        for lo, hi in shard_bounds(P, world, bs):
            parts.append(e.evaluate(x[lo:hi], generation=5, first_minibatch=lo // bs))
        F_shards = np.concatenate(parts)
        np.testing.assert_array_equal(F_shards, F_whole)       # kernel choice is a function of the layer geometry only (common.h)
    # an uneven split (3 ranks: 8 + 4 + 4) and a different generation both change nothing / something as expected
    parts = [e.evaluate(x[lo:hi], generation=5, first_minibatch=lo // bs) for lo, hi in shard_bounds(P, 3, bs)]
    np.testing.assert_array_equal(np.concatenate(parts), F_whole)
    assert np.abs(e.evaluate(x, generation=6) - F_whole).max() > 1e-5     # fresh noise per generation (modules.py:428-452)
    e.close()


def test_stream_modes_give_identical_results():
    """glass_engine_set_overlap: 0 = one stream, 1 = chunk pipelining, 2 = CLIP's image tower on a second stream next to the
    discriminator (the default).  The stream mode only moves launches between streams: fitness values are bit-identical."""
    name, P, bs = "mini", 16, 4
    c = M.CONFIGS[name]
    sd = M.make_state(name, 0)
    x = synth.latents(11, P, c["latent"])
    e = M.make_engine(name, sd, batch_size=bs, use_discriminator=True, max_pop=P, noise_mode=1, noise_seed=5, chunk=8)
    e.set_target(np.ones(c["clip"][5], np.float32))
    e.evaluate(x, generation=1)
    e.set_target(M.make_target(e.details(P)["features"]))
    ref = None
    for mode in (0, 2, 1, 2, 0):
        e.set_overlap(mode)
        for _ in range(2):
            F = e.evaluate(x, generation=3)
            if ref is None:
                ref = F
            np.testing.assert_array_equal(F, ref)
    e.close()


def test_launch_table_is_pinned():
    """Which kernel every layer runs on, in launch order: the profile's (row name, launches) list of one evaluate on two small networks
    against tests/golden/launch_table.json, recorded on the MI355X from the commit BEFORE the block walkers were rewritten.  A walker that
    falls back to a slower but correct path passes every parity test; it does not pass this one.  `mid` and `r128` (glass_models.py) are
    the smallest networks that reach the walkers' branches; the conditions below say which.  Not reachable at 128 px or below:
    conv_stream_kernel<torgb> (its admission wants 72 tiles per image: 256 px) and dblock0's chunk-planar output for conv_wreg (256 px) —
    so `ffhq` at one minibatch (P = 4: instance choice is made at the nominal population, so this is the benchmark's table) and `bg256`
    are pinned too, recorded from the commit BEFORE the conv families got their feature masks and choosers."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_table.json")) as f:
        golden = json.load(f)
    names = {k: [r[0] for r in rows] for k, rows in golden.items()}
    every = names["mid"] + names["r128"]

    def follows(rows, first, then):
        return any(first in a and then in b for a, b in zip(rows, rows[1:]))
    assert follows(names["r128"], "G.upconv.r128.64x64@upfir2_kernel", "G.conv.r128.64x64@conv_wreg_kernel")
    assert "G.conv.r32.512x512@conv_gldsp_kernel<true,false,false>" in every            # toRGB partial sums + finish
    assert any("torgb" in n and n.startswith("G.conv.") for n in every)                 # toRGB in the conv's epilogue
    assert any(n.startswith("G.torgb.") for n in every)                                 # separate toRGB
    assert any(n.endswith("@dblock0_kernel") for n in every)
    assert "D.conv0.r32.512x512@conv_gldsp_kernel<false,true,false>" in every and "D.blurdown.r32" not in every   # blur-down by-product
    assert any(n.startswith("D.conv1.") and n.endswith("@conv_s2_kernel") for n in every)               # fused skip
    assert any(n.startswith("D.conv1.") and n.endswith("skip>") for n in every)
    assert any(n.startswith("D.skip.") for n in every)                                  # separate skip + residual
    assert "D.fromrgb" in names["r128"] and any(n.startswith("D.blurdown.") for n in every)
    assert "G.conv.r1024.32x32@conv_stream_kernel<torgb>" in names["ffhq"]               # the map of the last G conv is never stored
    assert follows(names["ffhq"], "@dblock0_kernel", "D.conv0.r512.64x64@conv_wreg_kernel<false,true>")   # dblock0's chunk-planar output
    assert any(n.endswith("@conv_down64_kernel") for n in names["ffhq"])
    assert "bg.final.conv_to_rgb+tanh@conv_tiled_kernel<3,1,8,32>" in names["bg256"]    # the planar tanh: conv_tiled's alone
    for name in ("mid", "r128", "ffhq", "bg256"):
        if name in M.BIGGAN_CONFIGS:
            c = M.BIGGAN_CONFIGS[name]
            e = M.make_biggan_engine(name, M.make_biggan_state(name, 0), batch_size=4, max_pop=4)
            x = synth.biggan_population(1, 4, c["z_dim"], c["num_classes"])
        else:
            c = M.CONFIGS[name]
            e = M.make_engine(name, M.make_state(name, 0), batch_size=4, use_discriminator=True, max_pop=4, noise_mode=1)
            x = synth.latents(1, 4, c["latent"])
        e.set_target(np.ones(c["clip"][5], np.float32))
        e.set_profiling(True)
        e.evaluate(x)
        rows = [[r["name"], r["launches"]] for r in e.profile()]
        e.close()
        diff = [(i, a, b) for i, (a, b) in enumerate(zip(rows, golden[name])) if a != b]
        assert not diff and len(rows) == len(golden[name]), "%s: %d rows against %d pinned, first difference %r" % (
            name, len(rows), len(golden[name]), diff[:1])


def test_pop512_as_eight_shards_of_64():
    """BASELINE.json configs[3] (StyleGAN2_ffhq_d pop=512, 64 per GPU x 8) exercised as offset shards on ONE GPU at the mid
    architecture: the eight 64-row shard calls reproduce the whole-population call row for row."""
    from clip_glass_amd.parallel import shard_bounds
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mid_modules.npz"))
    name, P, bs = "mid", 512, 4
    c = M.CONFIGS[name]
    Pg = int(g["P"])
    sd = M.make_state(name, int(g["seed"]))
    # rows 0-7 = the reference-generated fixture's population (same seeds, device noise = the fixture's planes), so that C4 meets
    # the REFERENCE and not only itself; the other 504 rows are fresh latents
    x = np.concatenate([synth.latents(int(g["seed"]) + 1, Pg, c["latent"]), synth.latents(11, P - Pg, c["latent"])])
    e = M.make_engine(name, sd, batch_size=bs, use_discriminator=True, max_pop=P, noise_mode=1, noise_seed=int(g["noise_seed"]))
    e.set_target(g["target"])
    gen = int(g["generation"])
    F_whole = e.evaluate(x, generation=gen)
    det = e.details(P)
    parts = [e.evaluate(x[lo:hi], generation=gen, first_minibatch=lo // bs) for lo, hi in shard_bounds(P, 8, bs)]
    assert all(p.shape == (64, 2) for p in parts)
    Fs = np.concatenate(parts)
    for tag, Fx in (("whole", F_whole), ("shard 0", parts[0])):
        rel = np.abs(-Fx[:Pg, 0] - g["sim"]) / np.abs(g["sim"])
        diag("[e2e] pop512 %s rows 0-%d vs reference fixture: sim rel err %.3e, hinge abs err %.3e" % (tag, Pg - 1, rel.max(), np.abs(Fx[:Pg, 1] - g["hinge"]).max()))
        assert rel.max() < 1e-3
        check_logits("pop512 %s hinge rows 0-%d" % (tag, Pg - 1), Fx[:Pg, 1], g["hinge"], case="mid")
    check_logits("pop512 D logits rows 0-%d" % (Pg - 1), det["dis"][:Pg], g["dis"], case="mid")
    # every launch-size threshold in the dispatchers is evaluated at the nominal population (csrc/common.h GLASS_NOMINAL_POP), so a
    # 512-row launch and a 64-row launch run every layer on the same kernel instance with the same summation order: bitwise equal
    np.testing.assert_array_equal(Fs, F_whole)
    # the SAME 64-row launch repeated with the same offsets is bitwise reproducible
    again = e.evaluate(x[64:128], generation=gen, first_minibatch=16)
    np.testing.assert_array_equal(again, parts[1])
    e.close()


def test_bench_launcher_two_ranks_one_gpu():
    """`python bench.py --gpus 2` with WORLD_SIZE unset must become the launcher (torch.distributed.run, one process per
    rank) and print ONE JSON line with n_gpus = 2.  This box has one GPU: both ranks share it and rendezvous over gloo
    (GLASS_BENCH_BACKEND / GLASS_BENCH_SHARE_GPU are test knobs; the driver's 8-GPU run uses RCCL, one GPU per rank)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GLASS_BENCH_BACKEND="gloo", GLASS_BENCH_SHARE_GPU="1")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--config", "mid", "--pop", "8", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["config"]["global_pop"] == 16
    assert out["scaling"] == "weak" and out["value"] > 0


def test_full_size_ffhq_full_population():
    """The exact code path bench.py times: ffhq-1024 G+D + CLIP ViT-B/32, P = 64, default chunk (64), device noise.
    Rows 0-7 must equal the reference-generated fixture (tests/golden/ffhq_modules.npz, P = 8 = two minibatches), and the
    whole F must equal a chunk = 4 run (one minibatch per launch group) of the same population."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ffhq_modules.npz"))
    name, P, bs = "ffhq", 64, 4
    c = M.CONFIGS[name]
    Pg = int(g["P"])
    sd = M.make_state(name, int(g["seed"]))
    x = np.concatenate([synth.latents(int(g["seed"]) + 1, Pg, c["latent"]), synth.latents(1234, P - Pg, c["latent"])])
    Fs = []
    for chunk in (0, 4):
        e = M.make_engine(name, sd, batch_size=bs, use_discriminator=True, max_pop=P, noise_mode=1,
                          noise_seed=int(g["noise_seed"]), chunk=chunk)
        e.set_target(g["target"])
        Fs.append(e.evaluate(x, generation=int(g["generation"])))
        if chunk == 0:
            det = e.details(P)
        e.close()
    rel = np.abs(det["sim"][:Pg] - g["sim"]) / np.abs(g["sim"])
    diag("[e2e] ffhq P=64 default chunk: rows 0-%d vs reference fixture: sim rel err %.3e, D abs err %.3e; chunk 64 vs 4 max |dF| %.3e"
         % (Pg - 1, rel.max(), np.abs(det["dis"][:Pg] - g["dis"]).max(), np.abs(Fs[0] - Fs[1]).max()))
    assert rel.max() < 1e-3
    check_logits("ffhq P=64 D logits rows 0-%d" % (Pg - 1), det["dis"][:Pg], g["dis"], case="ffhq")
    assert np.isfinite(Fs[0]).all() and Fs[0].shape == (P, 2)
    # chunk 64 and chunk 4 launches run the same kernel instance per layer (dispatch looks at the layer geometry only): bitwise equal
    np.testing.assert_array_equal(Fs[0], Fs[1])


def test_full_size_offset_shards():
    """BASELINE.json configs[3] at the REAL architecture and the REAL population: ffhq-1024 G + D + CLIP ViT-B/32, P = 512 in ONE call
    against the eight 64-row shard calls the ranks of an 8-GPU job make (first_minibatch = 0, 16, ..., 112: rank r reads noise planes
    16 r .. 16 r + 15 and forms its own minibatch-stddev groups) — bitwise equal rows; rows 0-7 are the reference-generated fixture's
    population, checked against the fixture in the whole call AND in shard 0."""
    import os
    from clip_glass_amd.parallel import shard_bounds
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ffhq_modules.npz"))
    name, P, bs = "ffhq", 512, 4
    c = M.CONFIGS[name]
    Pg = int(g["P"])
    sd = M.make_state(name, int(g["seed"]))
    x = np.concatenate([synth.latents(int(g["seed"]) + 1, Pg, c["latent"]), synth.latents(4321, P - Pg, c["latent"])])
    e = M.make_engine(name, sd, batch_size=bs, use_discriminator=True, max_pop=P, noise_mode=1, noise_seed=int(g["noise_seed"]))
    e.set_target(g["target"])
    gen = int(g["generation"])
    F_whole = e.evaluate(x, generation=gen)
    det = e.details(P)
    bounds = shard_bounds(P, 8, bs)
    assert bounds == [(64 * r, 64 * r + 64) for r in range(8)]
    parts = [e.evaluate(x[lo:hi], generation=gen, first_minibatch=lo // bs) for lo, hi in bounds]
    for tag, Fx in (("whole", F_whole), ("shard 0", parts[0])):
        rel = np.abs(-Fx[:Pg, 0] - g["sim"]) / np.abs(g["sim"])
        diag("[e2e] ffhq P=512 %s rows 0-%d vs reference fixture: sim rel err %.3e, hinge abs err %.3e"
             % (tag, Pg - 1, rel.max(), np.abs(Fx[:Pg, 1] - g["hinge"]).max()))
        assert rel.max() < 1e-3
        check_logits("ffhq P=512 %s hinge rows 0-%d" % (tag, Pg - 1), Fx[:Pg, 1], g["hinge"], case="ffhq")
    check_logits("ffhq P=512 D logits rows 0-%d" % (Pg - 1), det["dis"][:Pg], g["dis"], case="ffhq")
    diag("[e2e] ffhq P=512 one call vs eight offset shards of 64: max |dF| %.3e" % np.abs(np.concatenate(parts) - F_whole).max())
    np.testing.assert_array_equal(np.concatenate(parts), F_whole)
    # a shard evaluated with the WRONG offset differs (its noise planes are another rank's): the offset is live
    assert np.abs(e.evaluate(x[64:128], generation=gen, first_minibatch=0) - parts[1]).max() > 1e-6
    e.close()


def test_rccl_two_ranks_all_gather():
    """The N > 1 product path on the REAL backend: two ranks, one GPU each, `nccl` (= RCCL) — shard scoring + the one all-gather of
    `[P/N, n_obj]` (parallel.py) against the whole population on one GPU, bitwise.  RCCL refuses two ranks on one device, so this
    runs on multi-GPU boxes only; the 1-GPU test boxes skip it WITH the reason (the gloo twin in tests/test_host.py and the offset-shard
    tests above cover the same arithmetic there)."""
    import json
    import os
    import socket
    import subprocess
    import sys
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("needs >= 2 GPUs (this box has %d): RCCL cannot place two ranks on one device; covered on 1-GPU boxes by the "
                    "gloo 2-rank tests and the bitwise offset-shard tests" % n)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(root, "tests", "rccl_worker.py")], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.strip().startswith("{")][-1])
    diag("[e2e] RCCL 2-rank all-gather: %r" % out)
    assert out["ok"] and out["backend"] == "nccl" and out["world"] == 2 and out["rows"] == 16
    assert out["gather_source"] == "device" and out["weak_scaling"]["rows_gathered"] == 128 and out["weak_scaling"]["finite"]


@pytest.mark.gpu
def test_rccl_one_rank_runs_the_collective():
    """What a 1-GPU box CAN run of the N > 1 path on the real backend: one rank under torch.distributed.run, `nccl` (= RCCL) initialised,
    `all_gather_into_tensor` executed on the engine's DEVICE-resident fitness rows (glass_engine_last_F_device: no D2H -> H2D bounce),
    even / ragged / weak-scaling forms against the whole population, bitwise — and bench.py's weak-scaling loop for 3 steps at the
    headline geometry through the same evaluator (the collective itself had never executed)."""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(root, "tests", "rccl_worker.py")], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.strip().startswith("{")][-1])
    diag("[e2e] RCCL 1-rank collective + weak-scaling loop: %r" % out)
    assert out["ok"] and out["backend"] == "nccl" and out["world"] == 1 and out["rows"] == 8 and out["gather_source"] == "device"
    w = out["weak_scaling"]
    assert w["rows_gathered"] == 64 and w["finite"] and w["gather_source"] == "device" and w["candidates_per_s"] > 500
