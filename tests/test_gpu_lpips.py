"""The perceptual objective end to end on the GPU: Engine.lpips against the float64 reference of tests/lpips_ref.py, and the fitness pass
with the distance as a third column / folded into the first.

The bar on the distance is not chosen here.  FP16_STORAGE_REL_* is the relative difference, measured on the CPU on these same inputs
(tests/test_lpips_ref.py reproduces it), between the float64 reference and the same arithmetic with the input, the weights and every stored
activation rounded to fp16 — what the storage format alone costs.  The GPU bar is twice that: the factor covers fp32 accumulation and the
summation order, which the CPU emulation does not model."""
import types

import numpy as np
import pytest
import torch

import glass_models as M
import lpips_ref as R
from clip_glass_amd import synth
from clip_glass_amd.engine import Engine, lpips_n_obj

FP16_STORAGE_REL_S32 = 5.13e-5      # max over the 3 fixture pairs at S = 32 (measured 5.122e-5)
FP16_STORAGE_REL_S16 = 5.27e-5      # the S = 16 pair (measured 5.269e-5)
GPU_BAR_S32 = 2 * FP16_STORAGE_REL_S32
GPU_BAR_S16 = 2 * FP16_STORAGE_REL_S16
# The existing end-to-end tests allow the engine's image an rms error of 1e-3 on the [0, 1] scale (tests/test_gpu_engine.py), 2e-3 on the raw
# [-1, 1] one.  What that does to the distance is measured on the reference: the largest change of d under seeded perturbations of that rms
# applied to the VGG input (a smooth error field passes the box mean undiminished).
IMAGE_RMS_ALLOWED = 2e-3


def inputs_s32():
    fx = np.load(R.FIXTURE)
    return fx["x32"].astype(np.float32), fx["t32"].astype(np.float32), synth.lpips_state(int(fx["seed"]))


def inputs_s16():
    return R.images(5, 1, 16, "a"), R.images(5, 1, 16, "b"), synth.lpips_state(R.FIXTURE_SEED)


def _engine(name, sd, lp_sd, *, lpips_size, lam=0.0, use_d=True, bs=2, max_pop=6, chunk=0, finalize=True):
    c = M.CONFIGS[name]
    n_obj = lpips_n_obj(use_d, lam) if lpips_size else (2 if use_d else 1)
    e = Engine(c["channels"][::-1], latent_size=c["latent"], mapping_layers=c["mapping"], batch_size=bs, use_discriminator=use_d,
               n_obj=n_obj, max_pop=max_pop, chunk=chunk, clip=c["clip"], noise_mode=2, mbstd_group=2, lpips_size=lpips_size,
               lpips_lambda=lam)
    e.load_state(sd)
    if lp_sd is not None:
        e.load_state(lp_sd)
    if finalize:
        e.finalize()
    return e


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ["s32_n3", "s16_n1"])
def test_engine_lpips_matches_float64_reference(case):
    (x0, x1, lp_sd), S, bar = (inputs_s32(), 32, GPU_BAR_S32) if case == "s32_n3" else (inputs_s16(), 16, GPU_BAR_S16)
    e = _engine("mini", M.make_state("mini", 0), lp_sd, lpips_size=S)
    got = e.lpips(x0, x1)
    same = e.lpips(x0, x0)
    e.close()
    ref = R.lpips(lp_sd, x0, x1)
    rel = np.abs(got - ref) / ref
    print("engine.lpips %s: d %s rel err %s (bar %.3e)" % (case, got, rel, bar))
    assert (same == 0).all()                    # identical images: exactly 0
    assert np.isfinite(got).all() and (rel <= bar).all()


def test_missing_tensor_and_missing_target_fail_by_name():
    sd, lp_sd = M.make_state("mini", 0), synth.lpips_state(1)
    short = {k: v for k, v in lp_sd.items() if k != "lpips.features.17.bias"}
    e = _engine("mini", sd, short, lpips_size=32, finalize=False)
    with pytest.raises(RuntimeError, match="missing tensor: lpips.features.17.bias"):
        e.finalize()
    e.close()
    e = _engine("mini", sd, lp_sd, lpips_size=32)
    e.set_target(np.ones(M.CONFIGS["mini"]["clip"][5], np.float32))
    x = synth.latents(1, 2, M.CONFIGS["mini"]["latent"])
    with pytest.raises(RuntimeError, match=r"set_lpips_target\(\) first"):
        e.evaluate(x, noise=M.noise_planes("mini", 7, 0, 1))
    with pytest.raises(ValueError, match="must be \\[3, 32, 32\\]"):
        e.set_lpips_target(np.zeros((3, 16, 16), np.float32))
    e.close()
    off = _engine("mini", sd, None, lpips_size=0)
    with pytest.raises(RuntimeError, match="perceptual objective is off"):
        off.last_lpips(2)
    off.close()


def _oracle_raw_images(name, sd, x, planes, bs):
    from oracle import stylegan2_ref as sg
    tsd = {k: torch.as_tensor(v) for k, v in sd.items()}
    z = torch.tensor(np.asarray(x).astype(float)).float()
    with torch.no_grad():
        return torch.cat([sg.generator(tsd, z[i * bs:(i + 1) * bs], planes[i]) for i in range(len(planes))]).numpy()


@pytest.mark.parametrize("name", ["mini", "mid"])           # 32 px (box 1) and 64 px (box 2) generators
def test_pass_with_the_distance_as_third_column(name):
    P, bs, S = 6, 2, 32
    c = M.CONFIGS[name]
    sd, lp_sd = M.make_state(name, 0), synth.lpips_state(3)
    x = synth.latents(4, P, c["latent"])
    planes = M.noise_planes(name, 7, 0, P // bs)
    tgt = R.images(9, 1, S, "target")[0]
    base = _engine(name, sd, None, lpips_size=0)
    base.set_target(np.ones(c["clip"][5], np.float32))
    base.evaluate(x, noise=planes)
    text = M.make_target(base.details(P)["features"])
    base.set_target(text)
    F0 = base.evaluate(x, noise=planes)
    base.close()
    assert F0.shape == (P, 2)

    e = _engine(name, sd, lp_sd, lpips_size=S)
    e.set_target(text)
    e.set_lpips_target(tgt)
    F1 = e.evaluate(x, noise=planes)
    d = e.last_lpips(P)
    assert F1.shape == (P, 3)
    assert F1[:, :2].tobytes() == F0.tobytes()              # the two existing columns: the same bits as without the objective
    assert F1[:, 2].tobytes() == d.tobytes()

    raw = _oracle_raw_images(name, sd, x, planes, bs)
    a = R.area(raw, S)
    ref = R.lpips(lp_sd, a, tgt[None])
    allow = np.zeros(P)
    for s in range(3):
        eta = synth.normal(20 + s, "eta", tuple(a.shape), std=IMAGE_RMS_ALLOWED)
        allow = np.maximum(allow, np.abs(R.lpips(lp_sd, a.numpy() + eta, tgt[None]) - ref))
    err = np.abs(d - ref)
    print("pass %s: d %s\n  err %s\n  bar %s (storage %.3e rel + image %s)" % (name, d, err, GPU_BAR_S32 * ref + allow, GPU_BAR_S32, allow))
    assert (err <= GPU_BAR_S32 * ref + allow).all()

    # rows do not depend on the chunk or the shard: the whole population (one chunk of 6) vs two chunks (4 + 2) vs offset shards
    e2 = _engine(name, sd, lp_sd, lpips_size=S, chunk=4)
    e2.set_target(text)
    e2.set_lpips_target(tgt)
    assert e2.evaluate(x, noise=planes).tobytes() == F1.tobytes()
    e2.close()
    parts = [e.evaluate(x[lo:hi], first_minibatch=lo // bs, noise=planes[lo // bs:hi // bs]) for lo, hi in ((0, 2), (2, 6))]
    assert np.concatenate(parts).tobytes() == F1.tobytes()
    e.close()

    # lambda > 0: no column, F[:, 0] = fma(lambda, d, -sim) to 1 ulp
    lam = 0.25
    e3 = _engine(name, sd, lp_sd, lpips_size=S, lam=lam)
    e3.set_target(text)
    e3.set_lpips_target(tgt)
    F3 = e3.evaluate(x, noise=planes)
    sim, d3 = e3.details(P)["sim"], e3.last_lpips(P)
    e3.close()
    assert F3.shape == (P, 2) and int(e3.cfg.n_obj) == 2
    assert d3.tobytes() == d.tobytes() and F3[:, 1].tobytes() == F0[:, 1].tobytes()
    want = (lam * d3.astype(np.float64) - sim.astype(np.float64)).astype(np.float32)
    assert (np.abs(F3[:, 0] - want) <= np.spacing(np.abs(want))).all()
    assert (F3[:, 0] != F0[:, 0]).all()


def test_a_chunk_longer_than_the_sub_chunk():
    """20 candidates in one chunk: the VGG walk takes them as 16 + 4 (GLASS_LPIPS_SUB); every distance equals the one of a pass over its
    own minibatch alone, bit for bit.  (The other two columns are compared with the engine without the objective at the same P: between
    launch sizes as far apart as 20 and 2 they agree to fp16 rounding only, which csrc/engine.cpp explains and this test is not about.)"""
    name, P, bs, S = "mini", 20, 2, 32
    c = M.CONFIGS[name]
    sd, lp_sd = M.make_state(name, 0), synth.lpips_state(3)
    x = synth.latents(6, P, c["latent"])
    planes = M.noise_planes(name, 7, 0, P // bs)
    base = _engine(name, sd, None, lpips_size=0, max_pop=P)
    base.set_target(np.ones(c["clip"][5], np.float32))
    F0 = base.evaluate(x, noise=planes)
    base.close()
    e = _engine(name, sd, lp_sd, lpips_size=S, max_pop=P)
    e.set_target(np.ones(c["clip"][5], np.float32))
    e.set_lpips_target(R.images(9, 1, S, "target")[0])
    F = e.evaluate(x, noise=planes)
    d = e.last_lpips(P)
    assert F.shape == (P, 3) and len(set(d.tolist())) == P
    assert F[:, :2].tobytes() == F0.tobytes() and F[:, 2].tobytes() == d.tobytes()
    for lo in (0, 14, 16, 18):
        Fm = e.evaluate(x[lo:lo + bs], first_minibatch=lo // bs, noise=planes[lo // bs:lo // bs + 1])
        assert Fm[:, 2].tobytes() == d[lo:lo + bs].tobytes(), lo
    e.close()


def test_profile_rows_without_the_objective_name_no_lpips_kernel():
    """lpips_size = 0: the pass launches what it launched before; with it on, the objective's rows appear next to the same list."""
    name, P, bs = "mini", 4, 2
    c = M.CONFIGS[name]
    sd, lp_sd = M.make_state(name, 0), synth.lpips_state(3)
    x = synth.latents(4, P, c["latent"])
    planes = M.noise_planes(name, 7, 0, P // bs)
    rows = {}
    for S in (0, 32):
        e = _engine(name, sd, lp_sd if S else None, lpips_size=S, max_pop=P)
        e.set_target(np.ones(c["clip"][5], np.float32))
        if S:
            e.set_lpips_target(R.images(9, 1, 32, "target")[0])
        e.set_overlap(0)
        e.set_profiling(True)
        e.evaluate(x, noise=planes)
        rows[S] = [(r["name"], r["launches"]) for r in e.profile()]
        e.close()
    assert not [n for n, _ in rows[0] if "lpips" in n]
    assert [r for r in rows[32] if "lpips" not in r[0]] == rows[0]
    got = {n.split("@")[0]: k for n, k in rows[32] if "lpips" in n}
    assert got["lpips.input"] == 1 and got["lpips.conv1"] == 1 and got["lpips.pool"] == 4 and got["lpips.head"] == 5
    assert sum(k for n, k in rows[32] if n.startswith("lpips.conv@")) == 12


def test_biggan_generation_problem_gets_a_second_objective(tmp_path):
    """DeepMindBigGAN config + lpips_target: n_obj 2 and nsga2 on the Generator's copy of the config, F [P, 2] = (-sim, d) through
    GenerationProblem._evaluate; the config table keeps n_obj 1 / ga."""
    from clip_glass_amd import config as gconfig
    from clip_glass_amd.problem import GenerationProblem
    c = M.BIGGAN_CONFIGS["bg_mini"]
    n_var = c["z_dim"] + c["num_classes"]
    x = synth.biggan_population(4, 8, c["z_dim"], c["num_classes"])
    tgt01 = (R.images(9, 1, 64, "bgt")[0] + 1) / 2
    extra = dict(weights="synthetic:0", clip_weights="synthetic:0", dim_z=c["z_dim"], num_classes=c["num_classes"],
                 biggan_geometry=dict(layers=c["layers"], attention_pos=c["attention_pos"], ch=c["ch"]),
                 clip_geometry=c["clip"], target_features=np.ones(c["clip"][5], np.float32), batch_size=4,
                 problem_args=dict(n_var=n_var, n_obj=1, n_constr=c["z_dim"], xl=-2, xu=2),
                 lpips_target=tgt01, lpips_size=32, lpips_weights="synthetic:3")
    cfg = types.SimpleNamespace(config="DeepMindBigGAN512", device="cuda", target="unused")
    vars(cfg).update(gconfig.get_config("DeepMindBigGAN512"))
    vars(cfg).update(extra)
    prob = GenerationProblem(cfg)
    assert prob.config.problem_args["n_obj"] == 2 and prob.config.algorithm == "nsga2" and prob.n_obj == 2
    assert cfg.problem_args["n_obj"] == 1 and gconfig.get_config("DeepMindBigGAN512")["algorithm"] == "ga"
    out = {}
    prob._evaluate(x.astype(object), out)
    assert out["F"].shape == (8, 2) and out["F"].dtype == np.float32
    d = prob.generator.engine.last_lpips(8)
    assert out["F"][:, 1].tobytes() == d.tobytes() and (d > 0).all() and np.isfinite(d).all()
    # the same distance from the engine's own images through the utility entry point: box 2 of the 64 px image is the 2 x 2 mean
    ls = cfg.latent(cfg)
    ls.set_from_population(x)
    img = prob.generator.generate(ls, minibatch=4)                      # [0, 1], clamped: tanh keeps BigGAN's raw output inside
    small = R.area(img * 2 - 1, 32).numpy().astype(np.float32)
    t = prob.generator.lpips_target
    again = prob.generator.engine.lpips(small, np.repeat(t[None], 8, axis=0))
    # (the [0, 1] round trip moves the input by fp32 roundings, which can flip fp16 roundings: each side is within the storage format's cost)
    assert (np.abs(again - d) <= 2 * GPU_BAR_S32 * d).all()
