"""What island populations cost and buy (DESIGN.md section 5 "Islands"): synthetic weights, ViT-B/32, one GPU.

    python tools/islands_cost.py [--cases ffhq:16:1,ffhq:16:2,ffhq:16:4,biggan:32:1,biggan:32:2] [--generations 20] [--quality-seeds 3]
                                 [--quality-generations 100] [--parent-lib PATH] [--out islands_cost.json]

cost (one child process per case WORKLOAD:POP:K).  ffhq = StyleGAN2 ffhq 1024 px + D, NSGA-II, batch 4; biggan = biggan-deep-512, GA, batch 8.
Wall time of one generation (search_step, median over --generations) of ONE engine with K islands of POP rows, against K times the generation of
a single-search engine of POP rows — K searches one after the other; then the profile rows (one stream, per-launch events) of survive,
migrate + re-rank (measured with migrate_every 1, 1 migrant) and noise as a share of the profiled pass.
quality (--quality-seeds > 0).  ffhq without D, GA, 64 rows per generation either way: 4 islands of 16 with ring migration of 1 row every 5
generations, 4 islands without migration, and one population of 64 — the best similarity after --quality-generations generations, per seed.
--parent-lib: a libglass.so built from the parent commit.  The feature-off pass (no search set; ffhq + D and biggan-deep-512 at P = 64) is
measured with it and with this tree's library in alternating processes.  Every measurement runs in a child process of this script."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ZD, NC = 128, 1000
VIT_B32 = (768, 12, 12, 32, 224, 512)
PASSES, WARM = 15, 3


def clip_state():
    from clip_glass_amd import synth
    return synth.make_state(synth.clip_visual_spec(VIT_B32[0], VIT_B32[1], VIT_B32[3], VIT_B32[4], VIT_B32[5]), 0)


def engine(workload, pop, islands, migrate_every=0, with_d=True, search=True, seed=1):
    """islands None: a single search of pop rows (the islands setter is never called)."""
    from clip_glass_amd import synth
    from clip_glass_amd.engine import Engine
    rows = pop * (islands or 1)
    if workload == "biggan":
        sd = synth.make_biggan_state(synth.biggan_spec(synth.BIGGAN_LAYERS[512], 8, 128, ZD, NC), 0)
        e = Engine([], batch_size=8, max_pop=rows, clip=VIT_B32,
                   biggan=dict(layers=synth.BIGGAN_LAYERS[512], attention_pos=8, ch=128, z_dim=ZD, num_classes=NC))
        if search:
            e.set_search_mixed("ga", pop, ZD, -2.0, 2.0, prob_x=0.2, prob_flip=10 / 1000, seed=seed)
    else:
        ch = synth.FFHQ_CHANNELS
        sd = synth.make_state(synth.stylegan2_g_spec(ch, 512, 8), 0)
        if with_d:
            sd.update(synth.make_state(synth.stylegan2_d_spec(ch), 0))
        e = Engine(ch[::-1], latent_size=512, mapping_layers=8, batch_size=4, use_discriminator=with_d, n_obj=2 if with_d else 1, max_pop=rows,
                   clip=VIT_B32, noise_mode=1, noise_seed=1234)
        if search:
            e.set_search("nsga2" if with_d else "ga", pop, -10.0, 10.0, seed=seed)
    if search and islands is not None:
        e.set_search_islands(islands, migrate_every, 1)
    sd.update(clip_state())
    e.load_state(sd)
    e.finalize()
    e.set_target(synth.normal(1, "t", (VIT_B32[5],)))
    return e


def population(workload, rows, seed=3):
    from clip_glass_amd import synth
    if workload == "biggan":
        x = synth.biggan_population(seed, rows, ZD, NC).astype(np.float32)
        x[:, :ZD] = np.clip(x[:, :ZD], -2.0, 2.0)
        x[:, ZD:] = np.random.default_rng(5 + seed).random((rows, NC)) < 0.005
        return x
    return synth.latents(seed, rows, 512)


def timed_generations(e, first, n):
    ms = []
    for g in range(first, first + n):
        t0 = time.perf_counter()
        e.search_step(g)
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def child_cost(workload, pop, K, generations):
    row = dict(kind="cost", workload=workload, pop=pop, islands=K, rows=pop * K)
    e = engine(workload, pop, K)
    e.search_init(population(workload, pop * K))
    timed_generations(e, 1, WARM)
    ms = timed_generations(e, 1 + WARM, generations)
    row.update(islands_generation_ms=float(np.median(ms)), islands_generation_ms_min=float(min(ms)), islands_generation_ms_max=float(max(ms)))
    e.close()
    e = engine(workload, pop, None)
    e.search_init(population(workload, pop))
    timed_generations(e, 1, WARM)
    ms = timed_generations(e, 1 + WARM, generations)
    row.update(single_generation_ms=float(np.median(ms)), single_generation_ms_min=float(min(ms)), single_generation_ms_max=float(max(ms)),
               k_singles_ms=float(np.median(ms)) * K)
    row["islands_vs_k_singles"] = row["islands_generation_ms"] / row["k_singles_ms"]
    e.close()
    # the phases: one stream, per-launch events, with a migration every generation
    e = engine(workload, pop, K, migrate_every=1)
    e.search_init(population(workload, pop * K))
    e.set_overlap(0)
    e.set_profiling(1)
    phases, total = {}, []
    for g in range(1, 6):
        e.search_step(g)
        rows = e.profile()
        total.append(sum(r["total_ms"] for r in rows if not r["name"].startswith("search.")))
        for r in rows:
            name = r["name"].split("@")[0]
            if name.startswith("search.") or name == "noise":
                phases.setdefault(name, []).append(r["total_ms"])
    row["profiled_pass_ms"] = float(np.median(total))
    row["phases_ms"] = {k: float(np.median(v)) for k, v in phases.items()}
    row["phases_share_of_pass"] = {k: float(np.median(v)) / row["profiled_pass_ms"] for k, v in phases.items()}
    row["accepted_last"] = [int(v) for v in e.search_read_islands()[:, 2]]
    e.close()
    print(json.dumps(row), flush=True)


def child_quality(seed, generations):
    """Equal evaluations: 64 rows per generation.  The same 64 initial rows everywhere: island i starts from rows [16 i, 16 i + 16)."""
    X0 = population("ffhq", 64, seed=10 + seed)
    out = dict(kind="quality", seed=seed, generations=generations, evaluations=64 * (generations + 1))
    for label, pop, K, M in (("islands_4x16_migrate_5", 16, 4, 5), ("islands_4x16_no_migration", 16, 4, 0), ("one_population_64", 64, None, 0)):
        e = engine("ffhq", pop, K, migrate_every=M, with_d=False, seed=seed)
        e.search_init(X0)
        for g in range(1, generations + 1):
            e.search_step(g)
        F = e.search_read("F")["F"]
        out[label] = float(-F[:, 0].min())      # the best similarity (F is its negative)
        if K:
            out[label + "_per_island"] = [float(-F[i * pop:(i + 1) * pop, 0].min()) for i in range(K)]
        e.close()
    print(json.dumps(out), flush=True)


def child_pass(label):
    """The feature-off pass (no search set) of whichever library GLASS_LIB names."""
    for workload in ("ffhq", "biggan"):
        e = engine(workload, 64, None, search=False)
        x = population(workload, 64)
        for g in range(WARM):
            e.evaluate(x, generation=g)
        ms = []
        for g in range(PASSES):
            e.evaluate(x, generation=WARM + g)
            ms.append(e.last_gpu_ms())
        e.close()
        print(json.dumps(dict(kind="pass", label=label, what=workload, P=64, pass_ms=float(np.median(ms)), pass_ms_min=float(min(ms)))), flush=True)


def run_child(args, what, lib=None):
    env = dict(os.environ)
    if lib:
        env["GLASS_LIB"] = os.path.abspath(lib)
    else:
        env.pop("GLASS_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--generations", str(args.generations),
                          "--quality-generations", str(args.quality_generations)], env=env, stdout=subprocess.PIPE, text=True, check=True, timeout=600)
    rows = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="ffhq:16:1,ffhq:16:2,ffhq:16:4,biggan:32:1,biggan:32:2")
    ap.add_argument("--generations", type=int, default=20)
    ap.add_argument("--quality-seeds", type=int, default=3)
    ap.add_argument("--quality-generations", type=int, default=100)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--pass-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        kind, *rest = args.child.split(":")
        if kind == "cost":
            return child_cost(rest[0], int(rest[1]), int(rest[2]), args.generations)
        if kind == "quality":
            return child_quality(int(rest[0]), args.quality_generations)
        return child_pass(rest[0])
    rows, passes, summary = [], [], []
    for case in filter(None, args.cases.split(",")):
        rows += run_child(args, "cost:" + case)
    for seed in range(1, args.quality_seeds + 1):
        rows += run_child(args, "quality:%d" % seed)
    if args.parent_lib:
        for r in range(args.pass_rounds):
            for label, lib in (("parent", args.parent_lib), ("this", None)):
                passes += [dict(q, round=r) for q in run_child(args, "pass:" + label, lib)]
        for what in ("ffhq", "biggan"):
            par = [q["pass_ms"] for q in passes if q["label"] == "parent" and q["what"] == what]
            this = [q["pass_ms"] for q in passes if q["label"] == "this" and q["what"] == what]
            ref = float(np.median(par))
            summary.append(dict(kind="summary", what=what, parent_pass_ms=ref, this_pass_ms=float(np.median(this)), parent_runs=par, this_runs=this,
                                parent_spread_rel=(max(par) - min(par)) / ref, this_vs_parent_rel=float(np.median(this)) / ref - 1.0))
        for s in summary:
            print(json.dumps(s), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(rows=rows, passes=passes, summary=summary), f, indent=1)


if __name__ == "__main__":
    main()
