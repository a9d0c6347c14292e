"""What a sep-CMA-ES generation costs around the pass, and what it buys (DESIGN.md section 5 "CMA-ES"): StyleGAN2 ffhq 1024 px without its
discriminator (one objective), ViT-B/32, synthetic weights, pop 64, batch 4, in z and in w+.

For each (space, algorithm in ga / cmaes): a device search of `--generations` generations per seed — the wall time of a generation
(callback to callback), the un-profiled pass on the GPU clock, the best similarity reached (equal evaluations: both score (generations + 1)
pop rows) — then the profile rows of the search's phases (one stream, per-launch events) as a share of the profiled pass.  With
--parent-lib (a libglass.so built from the parent commit) the feature-off pass, no search set, is measured with that library and with this
tree's in alternating processes.  Needs a GPU; every measurement runs in a child process of this script.

    python tools/cma_cost.py [--spaces z,w+] [--seeds 1,2,3] [--generations 100] [--parent-lib PATH] [--pass-rounds 3] [--out cma_cost.json]"""
import argparse
import json
import os
import subprocess
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
POP, BS = 64, 4
VIT_B32 = (768, 12, 12, 32, 224, 512)


class Problem:
    """The attributes search.minimize reads, over one engine."""

    def __init__(self, engine, n_var, xl, xu):
        self.engine, self.n_var, self.n_obj, self.xl, self.xu, self.ranks = engine, n_var, 1, xl, xu, 1
        self.config = types.SimpleNamespace(batch_size=BS)


class Sampling:
    """z ~ N(0, 1) from numpy's global generator; in w+ sent through the mapping network and repeated for every style layer."""

    def __init__(self, engine, space):
        self.engine, self.space = engine, space

    def _do(self, problem, n):
        z = np.random.normal(0, 1, size=(n, 512))
        if self.space == "z":
            return z
        w = np.concatenate([self.engine.map_latents(z[i:i + POP].astype(np.float32)) for i in range(0, n, POP)]).astype(float)
        return np.tile(w, (1, self.engine.latent_row()[1]))


def build_engine(space, algorithm):
    from clip_glass_amd import synth
    from clip_glass_amd.engine import Engine
    ch = synth.FFHQ_CHANNELS
    sd = synth.make_state(synth.stylegan2_g_spec(ch, 512, 8), 0)
    sd.update(synth.make_state(synth.clip_visual_spec(VIT_B32[0], VIT_B32[1], VIT_B32[3], VIT_B32[4], VIT_B32[5]), 0))
    e = Engine(ch[::-1], latent_size=512, mapping_layers=8, batch_size=BS, use_discriminator=False, n_obj=1, max_pop=POP, clip=VIT_B32,
               noise_mode=1, noise_seed=1234, latent_space=space)
    if algorithm:
        e.set_search(algorithm, POP, -10.0, 10.0, seed=1)
    e.load_state(sd)
    e.finalize()
    e.set_target(synth.normal(1, "t", (VIT_B32[5],)))
    return e


def child_search(space, algorithm, seeds, gens):
    from clip_glass_amd import search, synth
    e = build_engine(space, algorithm)
    xl, xu = -10.0, 10.0
    if space != "z":      # bounds half the mapped span beyond its extremes, exact in fp32 (problem.dlatent_problem_args's rule)
        w = e.map_latents(synth.latents(3, POP, 512).astype(np.float32))
        lo, hi = float(w.min()), float(w.max())
        xl, xu = float(np.float32(lo - (hi - lo) / 2)), float(np.float32(hi + (hi - lo) / 2))
    problem = Problem(e, e.latent_row()[0], xl, xu)
    row = dict(space=space, algorithm=algorithm, pop=POP, n_var=int(problem.n_var), generations=gens, best_similarity={})
    deltas, pass_ms = [], []
    for seed in seeds:
        stamps = []

        def tick(algo):
            stamps.append(time.perf_counter())
            pass_ms.append(e.last_gpu_ms())
        res = search.minimize(problem, algorithm, POP, gens, Sampling(e, space), seed=seed, callback=tick, device=True)
        deltas += list(np.diff(np.array(stamps)) * 1e3)
        row["best_similarity"][str(seed)] = -float(np.atleast_1d(res.F)[0])
        if algorithm == "cmaes":
            row.setdefault("sigma_last", {})[str(seed)] = float(res.sigma)
    row["generation_ms"] = float(np.median(deltas))
    row["generation_ms_min"], row["generation_ms_max"] = float(np.min(deltas)), float(np.max(deltas))
    row["generations_timed"] = len(deltas)
    row["pass_gpu_ms"] = float(np.median(pass_ms))
    e.set_overlap(0)      # the phases: one stream, per-launch events
    e.set_profiling(1)
    phases, total = {}, []
    for g in range(gens + 1, gens + 6):
        e.search_step(g)
        rows = e.profile()
        total.append(sum(r["total_ms"] for r in rows if not r["name"].startswith("search.")))
        for r in rows:
            if r["name"].startswith("search."):
                phases.setdefault(r["name"], []).append(r["total_ms"])
    e.set_profiling(0)
    row["profiled_pass_ms"] = float(np.median(total))
    row["phases_ms"] = {k: float(np.median(v)) for k, v in phases.items()}
    row["phases_share_of_pass"] = {k: float(np.median(v)) / row["profiled_pass_ms"] for k, v in phases.items()}
    e.close()
    print(json.dumps(row), flush=True)


def child_pass(label):
    """The feature-off pass (no search set) of whichever library GLASS_LIB names, at P = 64 in z."""
    from clip_glass_amd import synth
    e = build_engine("z", None)
    x = synth.latents(3, POP, 512).astype(np.float32)
    for g in range(3):
        e.evaluate(x, generation=g)
    ms = []
    for g in range(3, 18):
        e.evaluate(x, generation=g)
        ms.append(e.last_gpu_ms())
    e.close()
    print(json.dumps(dict(label=label, pass_ms=float(np.median(ms)), pass_ms_min=float(min(ms)))), flush=True)


def run_child(what, args, lib=None):
    env = dict(os.environ)
    if lib:
        env["GLASS_LIB"] = os.path.abspath(lib)
    else:
        env.pop("GLASS_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--seeds", args.seeds, "--generations", str(args.generations)],
                         env=env, stdout=subprocess.PIPE, text=True, check=True, timeout=600)
    rows = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spaces", default="z,w+")
    ap.add_argument("--seeds", default="1,2,3")
    ap.add_argument("--generations", type=int, default=100)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--pass-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        kind, _, rest = args.child.partition(":")
        if kind == "pass":
            return child_pass(rest)
        space, algorithm = rest.split(":")
        return child_search(space, algorithm, [int(s) for s in args.seeds.split(",")], args.generations)
    rows, passes = [], []
    for space in filter(None, args.spaces.split(",")):
        for algorithm in ("ga", "cmaes"):
            rows += run_child("search:%s:%s" % (space, algorithm), args)
    if args.parent_lib:
        for r in range(args.pass_rounds):
            for label, lib in (("parent", args.parent_lib), ("this", None)):
                passes += [dict(q, round=r) for q in run_child("pass:" + label, args, lib)]
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(pop=POP, batch_size=BS, rows=rows, passes=passes), f, indent=1)


if __name__ == "__main__":
    main()
