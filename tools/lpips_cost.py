"""What the perceptual objective costs (DESIGN.md section 5 "Perceptual objective"): the pass at the headline shape — StyleGAN2 ffhq 1024 px
with D, ViT-B/32, P = 64, batch 4, synthetic weights — with the objective off and on at S = 256 (box 4).  Per setting: the whole
un-profiled pass in the default stream mode (device time between the pass's own events, median of repeated passes after three warm-ups),
and with the objective on the lpips.* rows of a profiled one-stream pass (per-launch events; co-running kernels would stretch each other).
Needs a GPU.

    python tools/lpips_cost.py [--out lpips_cost.json] [--pop 64] [--passes 9]
"""
import argparse
import json
import os
import sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import glass_models as M
from clip_glass_amd import synth
from clip_glass_amd.engine import Engine, lpips_n_obj

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the figures and the per-launch rows to this JSON file")
ap.add_argument("--pop", type=int, default=64)
ap.add_argument("--passes", type=int, default=9)
ap.add_argument("--size", type=int, default=256)
args = ap.parse_args()
P, bs, S = args.pop, 4, args.size
c = M.CONFIGS["ffhq"]
sd = M.make_state("ffhq", 0)
lp_sd = synth.lpips_state(0)
x = synth.latents(3, P, c["latent"])
tgt = np.clip(synth.normal(5, "lpips_target", (3, S, S), std=0.4), -1, 1)
out = dict(P=P, S=S, passes=args.passes, settings={})
for on in (False, True):
    e = Engine(c["channels"][::-1], latent_size=c["latent"], mapping_layers=c["mapping"], batch_size=bs, use_discriminator=True,
               n_obj=lpips_n_obj(True, 0.0) if on else 2, max_pop=P, clip=c["clip"], noise_mode=1, lpips_size=S if on else 0)
    e.load_state(sd)
    if on:
        e.load_state(lp_sd)
    e.finalize()
    e.set_target(synth.normal(1, "t", (c["clip"][5],)))
    if on:
        e.set_lpips_target(tgt)
    for _ in range(3):
        e.evaluate(x)
    un = []
    for _ in range(args.passes):
        e.evaluate(x)
        un.append(e.last_gpu_ms())
    rows = []
    if on:
        e.set_overlap(0)
        e.set_profiling(1)
        e.evaluate(x)
        e.evaluate(x)
        rows = [r for r in e.profile() if r["name"].startswith("lpips.")]
        e.set_profiling(0)
    e.close()
    out["settings"]["on" if on else "off"] = dict(
        pass_ms_median=float(np.median(un)), pass_ms_min=float(min(un)), pass_ms_max=float(max(un)),
        lpips_rows_ms=float(sum(r["total_ms"] for r in rows)),
        rows=[dict(name=r["name"], launches=r["launches"], ms=round(r["total_ms"], 4), tflops=round(r["flops"] / max(r["total_ms"], 1e-9) / 1e9, 1),
                   gbs=round(r["bytes"] / max(r["total_ms"], 1e-9) / 1e6, 1)) for r in rows])
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
for k, v in out["settings"].items():
    print(json.dumps(dict(lpips=k, **{a: b for a, b in v.items() if a != "rows"})))
for r in out["settings"]["on"]["rows"]:
    print(r)
