"""What image editing costs (DESIGN.md section 5 "Image editing"): the flagship pass — StyleGAN2 ffhq 1024 px with its discriminator, ViT-B/32,
P = 64, synthetic weights — with the feature off (a prompt set of one entry through set_targets, today's kernels), with a direction source
and 0 views, with a direction source and 8 crop views (which includes the re-encoding of the source under every generation's boxes), and
with a direction source and the latent anchor as its own column.  Per case the whole un-profiled pass in the default stream mode, median of
repeated passes after warm-ups, every pass at a new generation.  Needs a GPU.

    python tools/edit_cost.py [--parent-lib PATH] [--rounds 2] [--out edit_cost.json]

--parent-lib: a libglass.so built from the commit before image editing.  Every round then measures it too (the feature-off cases only), in
a process of its own between the rounds of this tree's library, and the spread of its repeated runs is printed next to the difference — the
yardstick for "the feature-off pass is not slower".  Every measurement runs in a child process of this script (one library per process)."""
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
CASES = (("off", 0), ("off", 8), ("direction", 0), ("direction", 8), ("direction+anchor", 0))      # (what is on, crop views)


def child(label):
    from clip_glass_amd import synth
    from clip_glass_amd.engine import Engine, load_library
    has_edit = hasattr(load_library(), "glass_engine_set_direction_source")
    ch = synth.FFHQ_CHANNELS
    sd = synth.make_state(synth.stylegan2_g_spec(ch, 512, 8), 0)
    sd.update(synth.make_state(synth.stylegan2_d_spec(ch), 0))
    sd.update(synth.make_state(synth.clip_visual_spec(VIT_B32[0], VIT_B32[1], VIT_B32[3], VIT_B32[4], VIT_B32[5]), 0))
    x = synth.latents(3, P, 512)
    target = synth.normal(1, "t", (1, VIT_B32[5]))
    source = np.clip(synth.normal(2, "s", (3, 1024, 1024)) * 0.5, -1, 1).astype(np.float32)
    for what, V in CASES:
        if what != "off" and not has_edit:
            continue
        anchor = what.endswith("anchor")
        kw = dict(anchor=True) if anchor else {}
        e = Engine(ch[::-1], latent_size=512, mapping_layers=8, batch_size=BS, use_discriminator=True, n_obj=3 if anchor else 2, max_pop=P,
                   clip=VIT_B32, noise_mode=1, noise_seed=1234, clip_views=V, **kw)
        e.load_state(sd)
        e.finalize()
        e.set_targets(target, [1.0])
        if what != "off":
            e.set_direction_source(source)
        if anchor:
            e.set_anchor(x[0])
        e.set_overlap(2)
        for g in range(WARM):
            e.evaluate(x, generation=g)
        whole = []
        for g in range(PASSES):
            e.evaluate(x, generation=WARM + g)
            whole.append(e.last_gpu_ms())
        print(json.dumps(dict(label=label, what=what, views=V, pass_ms=float(np.median(whole)), pass_ms_min=float(min(whole)))), flush=True)
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
    for what, V in CASES:
        def runs(label, w):
            return [q["pass_ms"] for q in rows if q["label"] == label and q["what"] == w and q["views"] == V]
        base = runs("parent", "off") or runs("this", "off")
        ref = float(np.median(base))
        p = runs("this", what)
        summary.append(dict(what=what, views=V, pass_ms=float(np.median(p)), reference_pass_ms=ref,
                            reference="parent, feature off" if runs("parent", "off") else "this tree, feature off",
                            reference_spread_rel=(max(base) - min(base)) / ref, pass_vs_reference_rel=float(np.median(p)) / ref - 1.0))
    for s in summary:
        print(json.dumps(s))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(P=P, passes=PASSES, rows=rows, summary=summary), f, indent=1)


if __name__ == "__main__":
    main()
