"""What latent space "sub" costs and what it buys (DESIGN.md section 5 "Subspace search"): StyleGAN2 ffhq 1024 px, ViT-B/32, synthetic
weights, P = 64, batch 4.

  cost     with the discriminator (the flagship pass): for (G, K) in (1, 64), (3, 64), (18, 64), (1, 512), (18, 512) the `dlatents.sub` profile
           row of a single-stream instrumented pass, the rows of the whole mapping -> styles prefix next to it, and the un-instrumented pass
           in the default stream mode — medians of 12 after warm-ups; the w+ engine as the yardstick.
  pass     with --parent-lib (a libglass.so built from the parent commit): the feature-off pass (z, no setter called) of that library and of
           this tree's in alternating processes, as tools/edit_cost.py does.
  quality  without the discriminator (one objective), device search, seeds 1-3, 64 x (generations + 1) evaluations each: GA in z against GA
           in sub (one group, K = 64), sep-CMA-ES in w+ against sep-CMA-ES in sub (one group and three groups, K = 64).  The basis is the PCA
           of 4096 probed dlatents (subspace.pca_basis), the base their mean.  Synthetic towers: the numbers say how the algorithms move in
           each space, nothing about real prompts.

Needs a GPU; every measurement runs in a child process of this script (one library per process).

    python tools/subspace_cost.py [--what cost,pass,quality] [--parent-lib PATH] [--rounds 2] [--seeds 1,2,3] [--generations 100] [--out F.json]"""
import argparse
import json
import os
import subprocess
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P, BS, PASSES, WARM, L = 64, 4, 12, 3, 512
VIT_B32 = (768, 12, 12, 32, 224, 512)
SHAPES = ((1, 64), (3, 64), (18, 64), (1, 512), (18, 512))
GROUPS = {1: None, 3: "0-3,4-7,8-17", 18: ",".join(str(l) for l in range(18))}
PREFIX = ("mapping", "dlatents.sub", "dlatents", "styles", "demod", "premod_weights")


def state(with_d):
    from clip_glass_amd import synth
    ch = synth.FFHQ_CHANNELS
    sd = synth.make_state(synth.stylegan2_g_spec(ch, L, 8), 0)
    if with_d:
        sd.update(synth.make_state(synth.stylegan2_d_spec(ch), 0))
    sd.update(synth.make_state(synth.clip_visual_spec(VIT_B32[0], VIT_B32[1], VIT_B32[3], VIT_B32[4], VIT_B32[5]), 0))
    return ch, sd


def engine(ch, sd, with_d, search=None, **latent):
    from clip_glass_amd import synth
    from clip_glass_amd.engine import Engine
    e = Engine(ch[::-1], latent_size=L, mapping_layers=8, batch_size=BS, use_discriminator=with_d, n_obj=2 if with_d else 1, max_pop=P, clip=VIT_B32,
               noise_mode=1, noise_seed=1234, **latent)
    if search:
        e.set_search(search, P, -10.0, 10.0, seed=1)
    e.load_state(sd)
    e.finalize()
    e.set_target(synth.normal(1, "t", (VIT_B32[5],)))
    return e


def probed_basis(e, K, seed=0):
    """(basis [K][L], base [n_lat][L]) as generator.Generator builds them: PCA of 4096 probed dlatents, scaled to unit-variance coefficients."""
    from clip_glass_amd import subspace
    z = np.random.RandomState(seed).normal(size=(4096, L)).astype(np.float32)
    w = np.concatenate([e.map_latents(z[i:i + P]) for i in range(0, len(z), P)]).astype(np.float64)
    return subspace.operands(*subspace.pca_basis(w, K), e.latent_row()[1])


def timed(e, x):
    """(profile rows of the prefix, whole pass ms): medians over PASSES single-stream instrumented and default-mode passes."""
    for g in range(WARM):
        e.evaluate(x, generation=g)
    e.set_overlap(0)
    e.set_profiling(1)
    rows = []
    for g in range(PASSES):
        e.evaluate(x, generation=WARM + g)
        prof = e.profile()
        rows.append(dict({r["name"]: r["total_ms"] for r in prof if r["name"] in PREFIX}, profiled_pass=sum(r["total_ms"] for r in prof)))
    e.set_profiling(0)
    e.set_overlap(2)
    e.evaluate(x, generation=0)
    whole = []
    for g in range(PASSES):
        e.evaluate(x, generation=WARM + g)
        whole.append(e.last_gpu_ms())
    keys = sorted({k for r in rows for k in r})
    return {k: float(np.median([r.get(k, 0.0) for r in rows])) for k in keys}, float(np.median(whole))


def child_cost():
    from clip_glass_amd import subspace, synth
    ch, sd = state(True)
    e = engine(ch, sd, True, latent_space="w+")
    w = e.map_latents(synth.latents(3, P, L).astype(np.float32))
    rows, whole = timed(e, np.tile(w, (1, 18)))
    e.close()
    print(json.dumps(dict(kind="cost", space="w+", rows=rows, prefix_ms=sum(rows.get(k, 0.0) for k in PREFIX), pass_ms=whole)), flush=True)
    for G, K in SHAPES:
        e = engine(ch, sd, True, latent_space="sub", subspace_shape=(G, K))
        basis, base = probed_basis(e, K)
        e.set_subspace(subspace.parse_layer_groups(GROUPS[G], 18), basis, base)
        rows, whole = timed(e, np.random.RandomState(5).normal(size=(P, G * K)).astype(np.float32))
        e.close()
        print(json.dumps(dict(kind="cost", space="sub", G=G, K=K, rows=rows, sub_ms=rows["dlatents.sub"], prefix_ms=sum(rows.get(k, 0.0) for k in PREFIX),
                              pass_ms=whole, sub_share_of_pass=rows["dlatents.sub"] / whole,
                              basis_bytes=4 * K * L, fma=P * G * K * L)), flush=True)


def child_pass(label):
    from clip_glass_amd import synth
    ch, sd = state(True)
    e = engine(ch, sd, True)
    x = synth.latents(3, P, L).astype(np.float32)
    for g in range(WARM):
        e.evaluate(x, generation=g)
    ms = []
    for g in range(15):
        e.evaluate(x, generation=WARM + g)
        ms.append(e.last_gpu_ms())
    F = e.evaluate(x, generation=0)
    e.close()
    import hashlib
    print(json.dumps(dict(kind="pass", label=label, pass_ms=float(np.median(ms)), pass_ms_min=float(min(ms)),
                          F_sha256=hashlib.sha256(F.tobytes()).hexdigest())), flush=True)


class Problem:
    """The attributes search.minimize reads, over one engine."""

    def __init__(self, e, n_var, xl, xu):
        self.engine, self.n_var, self.n_obj, self.xl, self.xu, self.ranks = e, n_var, 1, xl, xu, 1
        self.config = types.SimpleNamespace(batch_size=BS)


class Sampling:
    """N(0, 1) rows from numpy's global generator: z and sub as they are, w+ through the mapping network and repeated for every layer."""

    def __init__(self, e, space):
        self.engine, self.space = e, space

    def _do(self, problem, n):
        if self.space == "sub":
            return np.random.normal(0, 1, size=(n, problem.n_var))
        z = np.random.normal(0, 1, size=(n, L))
        if self.space == "z":
            return z
        w = np.concatenate([self.engine.map_latents(z[i:i + P].astype(np.float32)) for i in range(0, n, P)]).astype(float)
        return np.tile(w, (1, self.engine.latent_row()[1]))


def child_quality(space, algorithm, G, seeds, gens):
    from clip_glass_amd import search, subspace, synth
    ch, sd = state(False)
    latent = dict(latent_space=space, subspace_shape=(G, 64)) if space == "sub" else dict(latent_space=space)
    e = engine(ch, sd, False, search=algorithm, **latent)
    xl, xu = -10.0, 10.0
    if space == "sub":
        basis, base = probed_basis(e, 64)
        e.set_subspace(subspace.parse_layer_groups(GROUPS[G], 18), basis, base)
    elif space != "z":      # bounds half the mapped span beyond its extremes, exact in fp32 (problem.dlatent_problem_args's rule)
        w = e.map_latents(synth.latents(3, P, L).astype(np.float32))
        lo, hi = float(w.min()), float(w.max())
        xl, xu = float(np.float32(lo - (hi - lo) / 2)), float(np.float32(hi + (hi - lo) / 2))
    problem = Problem(e, e.latent_row()[0], xl, xu)
    best = {}
    for seed in seeds:
        res = search.minimize(problem, algorithm, P, gens, Sampling(e, space), seed=seed, device=True)
        best[str(seed)] = -float(np.atleast_1d(res.F)[0])
    e.close()
    print(json.dumps(dict(kind="quality", space=space, algorithm=algorithm, groups=G if space == "sub" else None, n_var=int(problem.n_var),
                          evaluations=P * (gens + 1), best_similarity=best)), flush=True)


def run_child(what, args, lib=None):
    env = dict(os.environ)
    if lib:
        env["GLASS_LIB"] = os.path.abspath(lib)
    else:
        env.pop("GLASS_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--seeds", args.seeds, "--generations", str(args.generations)],
                         env=env, stdout=subprocess.PIPE, text=True, check=True, timeout=900)
    rows = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="cost,pass,quality")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--seeds", default="1,2,3")
    ap.add_argument("--generations", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        kind, _, rest = args.child.partition(":")
        if kind == "cost":
            return child_cost()
        if kind == "pass":
            return child_pass(rest)
        space, algorithm, G = rest.split(":")
        return child_quality(space, algorithm, int(G), [int(s) for s in args.seeds.split(",")], args.generations)
    what, rows = args.what.split(","), []
    if "cost" in what:
        rows += run_child("cost", args)
    if "pass" in what and args.parent_lib:
        for r in range(args.rounds):
            for label, lib in (("parent", args.parent_lib), ("this", None)):
                rows += [dict(q, round=r) for q in run_child("pass:" + label, args, lib)]
        par = [q["pass_ms"] for q in rows if q.get("label") == "parent"]
        new = [q["pass_ms"] for q in rows if q.get("label") == "this"]
        summary = dict(kind="pass_summary", parent_ms=float(np.median(par)), this_ms=float(np.median(new)), parent_spread_ms=max(par) - min(par),
                       this_minus_parent_ms=float(np.median(new)) - float(np.median(par)),
                       F_bitwise_equal=len({q["F_sha256"] for q in rows if q.get("kind") == "pass"}) == 1)
        print(json.dumps(summary), flush=True)
        rows.append(summary)
    if "quality" in what:
        for space, algorithm, G in (("z", "ga", 0), ("sub", "ga", 1), ("w+", "cmaes", 0), ("sub", "cmaes", 1), ("sub", "cmaes", 3)):
            rows += run_child("quality:%s:%s:%d" % (space, algorithm, G), args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(P=P, batch_size=BS, passes=PASSES, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
