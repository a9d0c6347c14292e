"""What the opt-in CLIP preprocessing costs on the headline workload (synthetic ffhq 1024 px, P = 64, ViT-B/32), in ONE process:
    python tools/preprocess_cost.py [--pop 64] [--rounds 12]
1. three engines ("reference", "antialias", "clip") and a second "reference" engine, alternated over --rounds un-instrumented populations
   each in the default stream mode: median last_gpu_ms per mode, and the spread of "reference" against itself;
2. one-stream profiled passes (set_overlap(0) + set_profiling): the `clip.resize` row of each mode, its bytes, and its time over
   bytes / 6.1 TB/s (the HBM read rate DESIGN.md section 5 measured);
3. the kernel row again for ViT-L/14@336 (1024 -> 336) through a 1-layer cut of that tower (the resize does not depend on the depth)."""
import argparse, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

HBM_TBS = 6.1
MODES = ["reference", "antialias", "clip"]


def build(E, synth, sd, clip, pop, mode, use_d=True):
    from clip_glass_amd.generator import CLIP_PREPROCESS
    rz, nm = CLIP_PREPROCESS[mode]
    eng = E.Engine(synth.FFHQ_CHANNELS[::-1], latent_size=512, mapping_layers=8, batch_size=4, use_discriminator=use_d,
                   n_obj=2 if use_d else 1, max_pop=pop, clip=clip, noise_mode=1, noise_seed=1234, clip_resize=rz, clip_normalize=nm)
    eng.load_state(sd)
    eng.finalize()
    eng.set_target(np.ones(clip[5], np.float32))
    return eng


def resize_row(eng, x, rounds=5):
    eng.set_overlap(0)
    eng.evaluate(x)
    us, nbytes = [], 0.0
    for r in range(rounds):
        eng.set_profiling(True)
        eng.evaluate(x, generation=r)
        for row in eng.profile():
            if row["name"] == "clip.resize":
                us.append(row["total_ms"] * 1e3)
                nbytes = row["bytes"]
        eng.set_profiling(False)
    eng.set_overlap(2)
    return float(np.median(us)), nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=12)
    a = ap.parse_args()
    from clip_glass_amd import synth, engine as E
    ch, clip = synth.FFHQ_CHANNELS, (768, 12, 12, 32, 224, 512)
    sd = synth.make_state(synth.stylegan2_g_spec(ch, 512, 8), 0)
    sd.update(synth.make_state(synth.stylegan2_d_spec(ch), 0))
    sd.update(synth.make_state(synth.clip_visual_spec(clip[0], clip[1], clip[3], clip[4], clip[5]), 0))
    names = MODES + ["reference#2"]
    engs = {n: build(E, synth, sd, clip, a.pop, n.split("#")[0]) for n in names}
    pops = [synth.latents(2000 + i, a.pop, 512) for i in range(a.rounds)]
    for n in names:                                   # warm-up: every engine, twice
        engs[n].evaluate(pops[0])
        engs[n].evaluate(pops[1 % len(pops)])
    ms = {n: [] for n in names}
    for i in range(a.rounds):
        for n in names:
            engs[n].evaluate(pops[i], generation=100 + i)
            ms[n].append(engs[n].last_gpu_ms())
    print("headline workload: ffhq 1024 px, P = %d, ViT-B/32, %d populations per engine, alternated; last_gpu_ms" % (a.pop, a.rounds))
    for n in names:
        v = np.array(ms[n])
        print("  %-12s median %8.3f ms   min %8.3f   max %8.3f" % (n, np.median(v), v.min(), v.max()))
    ref = float(np.median(ms["reference"]))
    print("  A/A spread (reference#2 - reference, medians): %+.3f ms" % (float(np.median(ms["reference#2"])) - ref))
    for n in MODES[1:]:
        print("  %-12s - reference: %+.3f ms (%+.2f %%)" % (n, float(np.median(ms[n])) - ref, (float(np.median(ms[n])) / ref - 1) * 100))
    print("clip.resize row, one stream, profiled (median of 5 passes; per pass of P = %d)" % a.pop)
    for n in MODES:
        us, nbytes = resize_row(engs[n], pops[0])
        floor = nbytes / (HBM_TBS * 1e12) * 1e6
        print("  %-12s 1024 -> 224  %9.1f us   %8.1f MB   floor %7.1f us   time / floor %5.2f" % (n, us, nbytes / 1e6, floor, us / floor))
    for n in names:
        engs[n].close()
    clip336 = (1024, 1, 16, 14, 336, 768)             # ViT-L/14@336's geometry, one layer deep
    sd336 = {k: v for k, v in sd.items() if not k.startswith("clip.")}
    sd336.update(synth.make_state(synth.clip_visual_spec(clip336[0], clip336[1], clip336[3], clip336[4], clip336[5]), 0))
    for n in MODES:
        eng = build(E, synth, sd336, clip336, a.pop, n)
        us, nbytes = resize_row(eng, pops[0])
        eng.close()
        floor = nbytes / (HBM_TBS * 1e12) * 1e6
        print("  %-12s 1024 -> 336  %9.1f us   %8.1f MB   floor %7.1f us   time / floor %5.2f" % (n, us, nbytes / 1e6, floor, us / floor))


if __name__ == "__main__":
    main()
