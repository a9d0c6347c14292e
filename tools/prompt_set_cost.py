"""What a prompt set costs (DESIGN.md section 5 "Prompt sets"): the flagship pass — StyleGAN2 ffhq 1024 px with its discriminator, ViT-B/32,
P = 64, synthetic weights — with one target through set_target (today's kernels) and with a set of T = 1, 4, 16 entries through set_targets,
views off and 8 views.  Per case: the clip.head profile row (one stream, per-launch events) and the whole un-profiled pass in the default
stream mode, median of repeated passes after warm-ups.  Needs a GPU.

    python tools/prompt_set_cost.py [--parent-lib PATH] [--rounds 2] [--out prompt_set_cost.json]

--parent-lib: a libglass.so built from the commit before prompt sets.  Every round then measures it too (its set_target case only), in a
process of its own between the rounds of this tree's library, and the spread of its repeated runs is printed next to the difference —
the yardstick for "not slower".  Every measurement runs in a child process of this script (one library per process)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P, BS, PASSES, WARM = 64, 4, 15, 3
VIT_B32 = (768, 12, 12, 32, 224, 512)
VIEWS, SETS = (0, 8), (1, 4, 16)


def child(label):
    from clip_glass_amd import synth
    from clip_glass_amd.engine import Engine, load_library
    has_sets = hasattr(load_library(), "glass_engine_set_targets")
    ch = synth.FFHQ_CHANNELS
    sd = synth.make_state(synth.stylegan2_g_spec(ch, 512, 8), 0)
    sd.update(synth.make_state(synth.stylegan2_d_spec(ch), 0))
    sd.update(synth.make_state(synth.clip_visual_spec(VIT_B32[0], VIT_B32[1], VIT_B32[3], VIT_B32[4], VIT_B32[5]), 0))
    x = synth.latents(3, P, 512)
    targets = synth.normal(1, "t", (16, VIT_B32[5]))
    weights = np.where(np.arange(16) % 3 == 1, -0.5, 1.0).astype(np.float32)
    for V in VIEWS:
        e = Engine(ch[::-1], latent_size=512, mapping_layers=8, batch_size=BS, use_discriminator=True, n_obj=2, max_pop=P, clip=VIT_B32,
                   noise_mode=1, noise_seed=1234, clip_views=V)
        e.load_state(sd)
        e.finalize()
        for T in (0,) + (SETS if has_sets else ()):          # 0: one target through set_target
            if T == 0:
                e.set_target(targets[0])
            else:
                e.set_targets(targets[:T], weights[:T])
            e.set_overlap(2)
            for _ in range(WARM):
                e.evaluate(x)
            whole = []
            for _ in range(PASSES):
                e.evaluate(x)
                whole.append(e.last_gpu_ms())
            e.set_overlap(0)
            e.set_profiling(1)
            head = []
            for _ in range(PASSES):
                e.evaluate(x)
                head.append(sum(r["total_ms"] for r in e.profile() if r["name"].split("@")[0] == "clip.head"))
            e.set_profiling(0)
            print(json.dumps(dict(label=label, views=V, T=T, pass_ms=float(np.median(whole)), pass_ms_min=float(min(whole)),
                                  head_ms=float(np.median(head)), head_ms_min=float(min(head)))), flush=True)
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    rows = []
    for r in range(args.rounds):
        for label, lib in (("parent", args.parent_lib), ("this", None)):
            if label == "parent" and not lib:
                continue
            env = dict(os.environ)
            if lib:
                env["GLASS_LIB"] = os.path.abspath(lib)
            else:
                env.pop("GLASS_LIB", None)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", label], env=env, stdout=subprocess.PIPE, text=True, check=True,
                                 timeout=900)
            for line in out.stdout.splitlines():
                if line.startswith("{"):
                    rows.append(dict(json.loads(line), round=r))
                    print(line, flush=True)
    summary = []
    for V in VIEWS:
        def runs(label, T, key):
            return [q[key] for q in rows if q["label"] == label and q["views"] == V and q["T"] == T]
        base = runs("parent", 0, "pass_ms") or runs("this", 0, "pass_ms")
        ref = float(np.median(base))
        spread = (max(base) - min(base)) / ref
        for T in (0,) + SETS:
            p, h = runs("this", T, "pass_ms"), runs("this", T, "head_ms")
            summary.append(dict(views=V, T=T, pass_ms=float(np.median(p)), head_ms=float(np.median(h)), reference_pass_ms=ref,
                                reference="parent" if runs("parent", 0, "pass_ms") else "this tree, set_target",
                                reference_spread_rel=spread, pass_vs_reference_rel=float(np.median(p)) / ref - 1.0))
    for s in summary:
        print(json.dumps(s))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(P=P, passes=PASSES, rows=rows, summary=summary), f, indent=1)


if __name__ == "__main__":
    main()
