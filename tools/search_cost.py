"""What a generation costs around the pass (DESIGN.md section 5 "Device search"): StyleGAN2 ffhq 1024 px with its discriminator, ViT-B/32,
synthetic weights, NSGA-II — wall time per generation of the host search (search.minimize: numpy selection, variation, duplicate elimination
and survival between two passes) and of the device search (search.minimize(device=True): one search_step), the un-profiled pass, and the
profile rows of the three new phases (one stream, per-launch events) as a share of the pass.  Needs a GPU.

    python tools/search_cost.py [--cases 64:z,64:w+,512:z] [--host-generations 4] [--device-generations 10] [--out search_cost.json]

The host search's code and the default pass are what they were before the device search existed, so the host column is also the parent
commit's generation on the same box.  Every case runs in a child process of this script."""
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
BS = 4
VIT_B32 = (768, 12, 12, 32, 224, 512)


class Problem:
    """The attributes search.minimize reads, over one engine."""

    def __init__(self, engine, n_var, xl, xu):
        self.engine, self.n_var, self.n_obj, self.xl, self.xu, self.ranks = engine, n_var, 2, xl, xu, 1
        self.config = types.SimpleNamespace(batch_size=BS)
        self.generation = 0

    def _evaluate(self, x, out):
        out["F"] = self.engine.evaluate(x, generation=self.generation)
        self.generation += 1


class Sampling:
    def __init__(self, X0):
        self.X0 = X0

    def _do(self, problem, n):
        return self.X0[:n] if n == self.X0.shape[0] else np.random.normal(size=(n, problem.n_var))


def child(pop, space, host_gens, dev_gens):
    from clip_glass_amd import search, synth
    from clip_glass_amd.engine import Engine
    ch = synth.FFHQ_CHANNELS
    sd = synth.make_state(synth.stylegan2_g_spec(ch, 512, 8), 0)
    sd.update(synth.make_state(synth.stylegan2_d_spec(ch), 0))
    sd.update(synth.make_state(synth.clip_visual_spec(VIT_B32[0], VIT_B32[1], VIT_B32[3], VIT_B32[4], VIT_B32[5]), 0))
    e = Engine(ch[::-1], latent_size=512, mapping_layers=8, batch_size=BS, use_discriminator=True, n_obj=2, max_pop=pop, clip=VIT_B32,
               noise_mode=1, noise_seed=1234, latent_space=space)
    e.set_search("nsga2", pop, -10.0, 10.0, seed=1)
    e.load_state(sd)
    e.finalize()
    e.set_target(synth.normal(1, "t", (VIT_B32[5],)))
    z = synth.latents(3, pop, 512)
    xl, xu = -10.0, 10.0
    if space == "z":
        X0 = z
    else:      # w+: every layer starts from the mapped row; bounds half the mapped span beyond its extremes, exact in fp32
        w = np.concatenate([e.map_latents(z[i:i + 64]) for i in range(0, pop, 64)])
        X0 = np.tile(w, (1, e.latent_row()[1]))
        lo, hi = float(w.min()), float(w.max())
        xl, xu = float(np.float32(lo - (hi - lo) / 2)), float(np.float32(hi + (hi - lo) / 2))
    problem = Problem(e, X0.shape[1], xl, xu)
    row = dict(pop=pop, space=space, n_var=int(X0.shape[1]))
    for device, gens in ((False, host_gens), (True, dev_gens)):
        stamps, pass_ms = [], []
        problem.generation = 0

        def tick(algo):
            stamps.append(time.perf_counter())
            pass_ms.append(e.last_gpu_ms())
        search.minimize(problem, "nsga2", pop, gens, Sampling(X0.astype(float)), seed=1, callback=tick, device=device)
        deltas = np.diff(np.array(stamps)) * 1e3      # callback to callback: generations 2 .. gens
        key = "device" if device else "host"
        row[key + "_generation_ms"] = float(np.median(deltas))
        row[key + "_generation_ms_min"] = float(deltas.min())
        row[key + "_generations_timed"] = int(deltas.size)
        row[key + "_pass_gpu_ms"] = float(np.median(pass_ms[1:]))
    # the three phases: one stream, per-launch events
    e.set_overlap(0)
    e.set_profiling(1)
    phases = {}
    total = []
    for g in range(dev_gens + 1, dev_gens + 6):
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
    row["counts_last"] = [int(v) for v in e.search_read("counts")["counts"]]
    e.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="64:z,64:w+,512:z")
    ap.add_argument("--host-generations", type=int, default=4)
    ap.add_argument("--device-generations", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        pop, space = args.child.split(":")
        return child(int(pop), space, args.host_generations, args.device_generations)
    rows = []
    for case in args.cases.split(","):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--host-generations", str(args.host_generations),
                              "--device-generations", str(args.device_generations)], stdout=subprocess.PIPE, text=True, check=True, timeout=900)
        for line in out.stdout.splitlines():
            if line.startswith("{"):
                rows.append(json.loads(line))
                print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(batch_size=BS, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
