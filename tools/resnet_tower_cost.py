"""What a CLIP ResNet image tower costs alone (DESIGN.md section 5 "ResNet towers"): RN50 at P = 64 with synthetic weights behind a mini
StyleGAN2, one stream, per-launch events, the sum of the clip.* profile rows of a pass (without clip.resize), median of repeated passes, and
the split by kernel family.  Needs a GPU.

    python tools/resnet_tower_cost.py [--out rn50_tower.json]
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
from clip_glass_amd.engine import Engine

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the figures and the per-launch rows to this JSON file")
args = ap.parse_args()
P, bs, PASSES = 64, 4, 11
RN50 = ((3, 4, 6, 3), 64, 224, 1024)
c = M.CONFIGS["mini"]
sd = synth.make_state(synth.stylegan2_g_spec(c["channels"], c["latent"], c["mapping"]), 0)
sd.update(synth.make_state(synth.clip_resnet_spec(*RN50), 0))
e = Engine(c["channels"][::-1], latent_size=c["latent"], mapping_layers=c["mapping"], batch_size=bs, use_discriminator=False, n_obj=1,
           max_pop=P, clip_resnet=RN50, noise_mode=1)
e.load_state(sd)
e.finalize()
e.set_target(synth.normal(1, "t", (1024,)))
e.set_overlap(0)
x = synth.latents(3, P, c["latent"])
for _ in range(3):
    e.evaluate(x)
e.set_profiling(1)
FAM = {"stem": ("clip.stem_conv",), "1x1": ("clip.rn_conv1", "clip.rn_conv3", "clip.rn_down"), "3x3": ("clip.rn_conv2",),
       "pools": ("clip.stem_pool", "clip.rn_pool"), "attention pool": ("clip.attnpool",)}
tot, fam, last = [], {k: [] for k in FAM}, None
for _ in range(PASSES):
    e.evaluate(x)
    rows = [r for r in e.profile() if r["name"].startswith("clip.") and not r["name"].startswith("clip.resize")]
    tot.append(sum(r["total_ms"] for r in rows))
    for k, pre in FAM.items():
        fam[k].append(sum(r["total_ms"] for r in rows if r["name"].startswith(pre)))
    last = rows
e.set_profiling(0)
un = []
for _ in range(PASSES):
    e.evaluate(x)
    un.append(e.last_gpu_ms())
out = dict(P=P, passes=PASSES, tower_ms_median=float(np.median(tot)), tower_ms_min=float(min(tot)), tower_ms_max=float(max(tot)),
           families_ms_median={k: float(np.median(v)) for k, v in fam.items()},
           whole_pass_unprofiled_ms_median=float(np.median(un)),
           rows=[dict(name=r["name"], launches=r["launches"], ms=round(r["total_ms"], 4), tflops=round(r["flops"] / max(r["total_ms"], 1e-9) / 1e9, 1),
                      gbs=round(r["bytes"] / max(r["total_ms"], 1e-9) / 1e6, 1)) for r in last])
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps({k: v for k, v in out.items() if k != "rows"}))
for r in out["rows"]:
    print(r)
e.close()
