"""What a BigGAN generation costs around the pass (DESIGN.md section 5 "Device search"): biggan-deep-512 with ViT-B/32, synthetic weights, GA,
batch 8 — wall time per generation of the host search (search.minimize: numpy selection, SBX / HUX / bit-flip, duplicate elimination and
survival between two passes) and of the device search on mixed rows (search.minimize(device=True): one search_step), the un-profiled pass,
and the profile rows of the search's phases (one stream, per-launch events) as a share of the pass.  Host and device searches alternate on
the same engine, `--rounds` times each.  Needs a GPU.

    python tools/search_cost_biggan.py [--cases 32,64] [--rounds 2] [--host-generations 6] [--device-generations 20]
                                       [--parent-lib PATH] [--out search_cost_biggan.json]

The host search's code is what it was before the device search took BigGAN rows, so the host column is also the parent commit's generation
on the same box.  --parent-lib: a libglass.so built from that commit.  The feature-off pass — BigGAN-512 and StyleGAN2 ffhq with its
discriminator, both at P = 64, no search set — is then measured with it and with this tree's library in alternating processes, and the
spread of the parent's own runs is printed next to the difference.  Every measurement runs in a child process of this script."""
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
BS, ZD, NC = 8, 128, 1000
VIT_B32 = (768, 12, 12, 32, 224, 512)
PASSES, WARM = 15, 3


def biggan_engine(pop, search):
    from clip_glass_amd import synth
    from clip_glass_amd.engine import Engine
    sd = synth.make_biggan_state(synth.biggan_spec(synth.BIGGAN_LAYERS[512], 8, 128, ZD, NC), 0)
    sd.update(synth.make_state(synth.clip_visual_spec(VIT_B32[0], VIT_B32[1], VIT_B32[3], VIT_B32[4], VIT_B32[5]), 0))
    e = Engine([], batch_size=BS, max_pop=pop, clip=VIT_B32, biggan=dict(layers=synth.BIGGAN_LAYERS[512], attention_pos=8, ch=128, z_dim=ZD, num_classes=NC))
    if search:
        e.set_search_mixed("ga", pop, ZD, -2.0, 2.0, prob_x=0.2, prob_flip=10 / 1000, seed=1)
    e.load_state(sd)
    e.finalize()
    e.set_target(synth.normal(1, "t", (VIT_B32[5],)))
    return e


def population(pop):
    from clip_glass_amd import synth
    x = synth.biggan_population(3, pop, ZD, NC).astype(np.float64)
    x[:, :ZD] = np.clip(x[:, :ZD], -2.0, 2.0)
    x[:, ZD:] = np.random.default_rng(5).random((pop, NC)) < 0.005
    return x


class Problem:
    """The attributes search.minimize reads, over one engine."""

    def __init__(self, engine):
        self.engine, self.n_var, self.n_obj, self.xl, self.xu, self.ranks = engine, ZD + NC, 1, -2.0, 2.0, 1
        self.config = types.SimpleNamespace(batch_size=BS)

    def _evaluate(self, x, out):
        out["F"] = self.engine.evaluate(np.asarray(x, np.float32))


class Sampling:
    def __init__(self, X0):
        self.X0 = X0

    def _do(self, problem, n):
        if n == self.X0.shape[0]:
            return self.X0
        return np.concatenate([np.clip(np.random.normal(size=(n, ZD)), -2, 2), (np.random.random((n, NC)) < 0.005).astype(float)], axis=1)


def child_search(pop, rounds, host_gens, dev_gens):
    from clip_glass_amd import search
    e = biggan_engine(pop, True)
    problem, X0 = Problem(e), population(pop)
    mask = ["real"] * ZD + ["bool"] * NC
    row = dict(pop=pop, batch_size=BS, n_var=ZD + NC)
    deltas, passes = dict(host=[], device=[]), dict(host=[], device=[])
    for _ in range(rounds):
        for device, gens in ((False, host_gens), (True, dev_gens)):
            stamps, pass_ms = [], []

            def tick(algo):
                stamps.append(time.perf_counter())
                pass_ms.append(e.last_gpu_ms())
            search.minimize(problem, "ga", pop, gens, Sampling(X0), seed=1, callback=tick, mask=mask, device=device)
            key = "device" if device else "host"
            deltas[key] += (np.diff(np.array(stamps)) * 1e3).tolist()      # callback to callback: generations 2 .. gens
            passes[key] += pass_ms[1:]
    for key in ("host", "device"):
        d = np.array(deltas[key])
        row[key + "_generation_ms"] = float(np.median(d))
        row[key + "_generation_ms_min"] = float(d.min())
        row[key + "_generation_ms_max"] = float(d.max())
        row[key + "_generations_timed"] = int(d.size)
        row[key + "_pass_gpu_ms"] = float(np.median(passes[key]))
    # the search's phases: one stream, per-launch events
    e.set_overlap(0)
    e.set_profiling(1)
    phases, total = {}, []
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


def timed_passes(e, x, label, what):
    for g in range(WARM):
        e.evaluate(x, generation=g)
    ms = []
    for g in range(PASSES):
        e.evaluate(x, generation=WARM + g)
        ms.append(e.last_gpu_ms())
    print(json.dumps(dict(label=label, what=what, P=int(x.shape[0]), pass_ms=float(np.median(ms)), pass_ms_min=float(min(ms)))), flush=True)


def child_pass(label):
    """The feature-off pass (no search set) of whichever library GLASS_LIB names: BigGAN-512 and StyleGAN2 ffhq with D, both at P = 64."""
    from clip_glass_amd import synth
    from clip_glass_amd.engine import Engine
    e = biggan_engine(64, False)
    timed_passes(e, population(64).astype(np.float32), label, "biggan512")
    e.close()
    ch = synth.FFHQ_CHANNELS
    sd = synth.make_state(synth.stylegan2_g_spec(ch, 512, 8), 0)
    sd.update(synth.make_state(synth.stylegan2_d_spec(ch), 0))
    sd.update(synth.make_state(synth.clip_visual_spec(VIT_B32[0], VIT_B32[1], VIT_B32[3], VIT_B32[4], VIT_B32[5]), 0))
    e = Engine(ch[::-1], latent_size=512, mapping_layers=8, batch_size=4, use_discriminator=True, n_obj=2, max_pop=64, clip=VIT_B32, noise_mode=1,
               noise_seed=1234)
    e.load_state(sd)
    e.finalize()
    e.set_target(synth.normal(1, "t", (VIT_B32[5],)))
    timed_passes(e, synth.latents(3, 64, 512), label, "stylegan2_ffhq")
    e.close()


def run_child(args, what, lib=None):
    env = dict(os.environ)
    if lib:
        env["GLASS_LIB"] = os.path.abspath(lib)
    else:
        env.pop("GLASS_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--rounds", str(args.rounds), "--host-generations",
                          str(args.host_generations), "--device-generations", str(args.device_generations)], env=env, stdout=subprocess.PIPE,
                         text=True, check=True, timeout=900)
    rows = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="32,64")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--host-generations", type=int, default=6)
    ap.add_argument("--device-generations", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--pass-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        kind, arg = args.child.split(":")
        return child_search(int(arg), args.rounds, args.host_generations, args.device_generations) if kind == "search" else child_pass(arg)
    rows = []
    for case in filter(None, args.cases.split(",")):
        rows += run_child(args, "search:" + case)
    passes, summary = [], []
    if args.parent_lib:
        for r in range(args.pass_rounds):
            for label, lib in (("parent", args.parent_lib), ("this", None)):
                passes += [dict(q, round=r) for q in run_child(args, "pass:" + label, lib)]
        for what in ("biggan512", "stylegan2_ffhq"):
            par = [q["pass_ms"] for q in passes if q["label"] == "parent" and q["what"] == what]
            this = [q["pass_ms"] for q in passes if q["label"] == "this" and q["what"] == what]
            ref = float(np.median(par))
            summary.append(dict(what=what, parent_pass_ms=ref, this_pass_ms=float(np.median(this)), parent_runs=par, this_runs=this,
                                parent_spread_rel=(max(par) - min(par)) / ref, this_vs_parent_rel=float(np.median(this)) / ref - 1.0))
        for s in summary:
            print(json.dumps(s), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(rows=rows, passes=passes, summary=summary), f, indent=1)


if __name__ == "__main__":
    main()
