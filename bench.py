#!/usr/bin/env python
"""bench.py — candidates scored per second through the MI355X fitness engine.

Workload (BASELINE.json configs[1]): StyleGAN2_ffhq_d — StyleGAN2 ffhq config-f 1024 px
generator + discriminator + CLIP ViT-B/32, pop = 64 per GPU, batch_size = 4 (noise
sharing / mbstd groups as in the reference config.py:80-95), n_obj = 2.  A "step" is
one `_evaluate` of one population (problem.py:14-29).  Synthetic seeded weights of the
true architecture (no checkpoints in this environment), fresh N(0,1) latents per step.

  python bench.py --gpus N --steps K --warmup W      (N > 1: launched by torch.distributed.run)

Prints ONE JSON line on rank 0.  Multi-GPU: the population shards across ranks (weak
scaling, 64 candidates per GPU) and the only collective is one RCCL all-gather of the
[P/N, n_obj] fitness rows per step.

A plain run sets up, warms up, times K steps and prints the headline line (metric, value,
unit, higher_is_better, dtype, ms_per_step); nothing in it is instrumented.  `--full` adds
what takes runs or passes of its own: the per-kernel roofline (profiled warm-up, dominant
kernel instrumented in the timed region, one single-stream instrumented pass after it), the
CPU baseline, the biggan512 / gpt2 legs and the GLASS_BENCH_DETAIL dump.
`--dump-outputs DIR` writes the fitness rows F of the last timed step to DIR/fitness.npy
(float32 [P * N, n_obj]); the inputs are seeded, so two builds compare output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "candidate latents scored/sec (GAN→CLIP fitness), StyleGAN2_ffhq_d pop=64"
MFMA_PEAK_TFLOPS = 2500.0   # dense f16/bf16 MFMA peak, MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0       # HBM3E spec peak, MI355X_MICROARCH.md
HBM_ACHIEVABLE_GBS = 6300.0 # measured achievable (float4 copy, 79 %): the rate roofline.families' roof_ms column prices bytes at
POP, BATCH = 64, 4


# engine kernel labels name template FLAGS by word; rocprofv3 prints every template argument: flag positions per kernel family
_FLAG_ARGS = {"conv_stream_kernel": (0, ["fromrgb", "torgb", "trace"]),
              "conv_tiled_kernel": (4, ["persist", "torgb", "skip", "xs", "spl", "b2", "deep", "tr"])}
# launches the engine tags by LAYER only (no "@kernel" part): the kernel symbol they run on
_TAG_KERNELS = (("D.blurdown.", "blur_kernel<1,2,8>"), ("D.blur.", "blur_kernel<2,1,16>"), ("G.torgb.", "torgb_kernel<64>"), ("noise", "noise_kernel"), ("clip.layernorm", "layernorm_kernel"),
                ("clip.attention", "attention_mfma_kernel<2>"), ("clip.resize", "resize_patches_kernel"),
                ("clip.embed_lnpre", "embed_lnpre_kernel"), ("mapping", "mapping_fused_kernel<2>"), ("D.mbstd", "mbstd_vec_kernel"),
                ("styles", "dense_kernel"), ("demod", "dense_kernel"), ("premod_weights", "modulate_weights_kernel"))


def _canon_symbol(sym):
    """A rocprofv3 kernel name (demangled `name<args>`, or still mangled `_Z<len><name>I..E...` when the signature holds a
    _Float16 pointer the demangler does not know) -> (base name, [template args as strings])."""
    import re
    sym = sym.replace(" ", "")
    m = re.match(r"_Z(\d+)", sym)
    if m:
        n = int(m.group(1))
        base = sym[m.end():m.end() + n]
        rest = sym[m.end() + n:]
        args = []
        if rest.startswith("I"):
            for kind, val in re.findall(r"L([ib])(\d+)E", rest[1:rest.index("EE") + 1] if "EE" in rest else rest):
                args.append(val if kind == "i" else ("true" if val == "1" else "false"))
        return base, args
    base, _, args = sym.partition("<")
    return base, [x for x in args.rstrip(">").split(",") if x]


def _canon_label(name):
    """An engine kernel label (`conv_tiled_kernel<3,1,8,64,xs,deep>`, or a bare layer tag such as `D.blur.r512`) -> the same pair."""
    for prefix, kern in _TAG_KERNELS:
        if name.startswith(prefix):
            name = kern
            break
    base, args = _canon_symbol(name)
    if base in _FLAG_ARGS and any(not (a.isdigit() or a in ("true", "false")) for a in args):
        n_lead, flags = _FLAG_ARGS[base]
        words = set(args[n_lead:])
        assert words <= set(flags), (name, words)
        args = args[:n_lead] + ["true" if f in words else "false" for f in flags]
    return base, args


def kernel_family(name):
    """`<layer tag>@<kernel symbol>` -> the kernel's SOURCE name (template arguments dropped): the dominant kernel of the `roofline` block is
    the source kernel with the largest share of device time — `conv_gldsp_kernel<true,false,false>` / `<false,true,false>` are one kernel
    with two epilogues (round 6: as separate symbols each was smaller than `dblock0_kernel` and the block would have named that one)."""
    kern = name.split("@")[1] if "@" in name else name
    return kern.split("<")[0]


def match_family(base, table):
    """Launch-weighted PMC row of ALL template instances of a source kernel in a {rocprofv3 symbol: row} table."""
    rows = [row for sym, row in table.items() if _canon_symbol(sym)[0] == base]
    n = sum(r["launches"] for r in rows)
    if not n:
        return None
    return dict(bytes_per_launch=sum(r["bytes_per_launch"] * r["launches"] for r in rows) / n, launches=n)


def match_kernel(name, table):
    """Row of a {rocprofv3 kernel symbol: row} table (tools/traffic_table.py) for an engine kernel label: same base name, and the
    label's template arguments a prefix of the symbol's (rocprofv3 also prints defaulted arguments).  Every label of the top-10
    kernels resolves (four of them silently got `traffic: null`); tests/test_host.py pins the map on the stored table."""
    b0, a0 = _canon_label(name)
    for sym, row in table.items():
        b1, a1 = _canon_symbol(sym)
        if b0 == b1 and a1[:len(a0)] == a0:
            return row
    return None


def family_table(iso, step_ms, traffic_rows, top=12):
    """Time-weighted per-kernel table of ONE instrumented single-stream pass: share of the pass, algorithmic TFLOP/s and GB/s with
    their fractions of the MFMA / HBM peaks, PMC traffic per launch over the algorithmic bytes (stored table) — the dominant
    family alone holds ~13 % of the step (report all of them, not one)."""
    tot = sum(v["total_ms"] for v in iso.values()) or 1.0
    rows = []
    for kern, v in sorted(iso.items(), key=lambda kv: -kv[1]["total_ms"])[:top]:
        secs = v["total_ms"] * 1e-3
        tf, gbs = v["flops"] / secs / 1e12, v["bytes"] / secs / 1e9
        tr = match_kernel(kern, traffic_rows) if traffic_rows else None
        alg_bpl = v["bytes"] / max(v["launches"], 1)
        # roof_ms: the family's distance-to-roof column = max(flop / MFMA peak, algorithmic bytes / ACHIEVABLE HBM rate)
        roof_ms = max(v["flops"] / (MFMA_PEAK_TFLOPS * 1e12), v["bytes"] / (HBM_ACHIEVABLE_GBS * 1e9)) * 1e3
        rows.append(dict(kernel=kern, launches=v["launches"], ms=round(v["total_ms"], 3), share=round(v["total_ms"] / tot, 4),
                         roof_ms=round(roof_ms, 3), x_roof=round(v["total_ms"] / roof_ms, 2) if roof_ms > 0 else None,
                         tflops=round(tf, 1), frac_mfma=round(tf / MFMA_PEAK_TFLOPS, 4), gbs=round(gbs, 1), frac_hbm=round(gbs / HBM_PEAK_GBS, 4),
                         traffic_ratio=(round(tr["bytes_per_launch"] / alg_bpl, 3) if tr and alg_bpl else None)))
    covered = sum(r["ms"] for r in rows)
    return dict(rows=rows, pass_ms=round(tot, 3), covered_share=round(covered / tot, 4), roof_ms_sum=round(sum(r["roof_ms"] for r in rows), 3),
                time_weighted_frac_mfma=round(sum(r["frac_mfma"] * r["ms"] for r in rows) / covered, 4) if covered else None,
                note="one single-stream pass with every launch instrumented (after the timed region); traffic_ratio = stored PMC bytes "
                     "per launch / algorithmic bytes per launch (kernel average over its layers)")


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, **arrays):
    """--dump-outputs: each array as <path>/<name>.npy in float32 (float64 stays float64), 64 MB at most in all."""
    os.makedirs(path, exist_ok=True)
    arrays = {k: np.asarray(v, np.float64 if np.asarray(v).dtype == np.float64 else np.float32) for k, v in arrays.items()}
    assert sum(v.nbytes for v in arrays.values()) <= DUMP_LIMIT_BYTES, "outputs exceed the 64 MB dump limit"
    for name, v in arrays.items():
        np.save(os.path.join(path, name + ".npy"), v)


def cpu_baseline(sd, cfg, target, pop=BATCH, budget_s=150.0, threads=(8, 16, 32, 64, 128)):
    """the oracle (CPU restatement of problem.py:14-29, kind 'port') on this box's host cores, same
    synthetic weights / batch_size-4 grouping / fixed noise planes as the GPU run, fp32.  torch's intra-op thread count is SWEPT
    once (one timed `_evaluate` per count after a warm-up call; counts above the box's cores are skipped; the sweep walks on downward by
    halves while its lower edge is the best) and the best count is reported with the median of up to 3 FRESH calls and the per-stage
    split (G / CLIP / D) — an oversubscribed pool is not the
    reference's CPU path timed properly.  Bounded sample: `pop` candidates (default one minibatch of 4;
    --cpu-baseline-pop 64 times the whole headline population); the extra calls stop once `budget_s` is spent."""
    import torch
    from clip_glass_amd import synth
    from oracle import fitness_ref
    tsd = {k: torch.as_tensor(v) for k, v in sd.items()}
    x_all = synth.latents(123, pop, cfg["latent"])
    planes = synth.g_noise_planes(9, 0, 0, cfg["channels"])

    def one_call(rows=None):
        x = x_all if rows is None else x_all[:rows]
        with torch.no_grad():
            t0 = time.time()
            img = fitness_ref.generate(tsd, x, BATCH, lambda i: planes)
            t1 = time.time()
            fitness_ref.clip_similarity(tsd, img, target, cfg["clip"][4])
            t2 = time.time()
            fitness_ref.discriminate(tsd, img, BATCH)
            t3 = time.time()
        return t3 - t0, t1 - t0, t2 - t1, t3 - t2
    try:
        import psutil
        phys = psutil.cpu_count(logical=False)
    except Exception:
        phys = None
    ncpu = os.cpu_count() or 1
    default_threads = torch.get_num_threads()
    counts = sorted({n for n in threads if n <= ncpu} | ({min(default_threads, ncpu)} if len(threads) > 1 else set())) or [ncpu]
    t_begin = time.time()
    torch.set_num_threads(counts[-1])
    one_call(BATCH)                                       # warm-up on one minibatch (allocator, thread pool, oneDNN primitive caches)
    sweep = {}
    for n in counts:
        torch.set_num_threads(n)
        sweep[n] = one_call()
        if time.time() - t_begin > budget_s and len(sweep) >= 2:
            break
    best = min(sweep, key=lambda n: sweep[n][0])
    # the optimum may lie BELOW the sweep (the best count was its lower edge): walk down by halves while that keeps paying
    while len(threads) > 1 and best == min(sweep) and best > 1 and time.time() - t_begin < budget_s:
        n = best // 2
        torch.set_num_threads(n)
        sweep[n] = one_call()
        best = min(sweep, key=lambda k: sweep[k][0])
    torch.set_num_threads(best)
    # fresh calls for the reported median (the sweep's own sample of the winner was selected for being the minimum: biased low)
    calls = []
    while len(calls) < 3 and (not calls or time.time() - t_begin < budget_s):
        calls.append(one_call())
    torch.set_num_threads(default_threads)
    med = [float(np.median([c[i] for c in calls])) for i in range(4)]
    return dict(value=pop / med[0], unit="candidates/s", cores=best, physical_cores=phys, logical_cpus=ncpu, kind="port",
                seconds_per_evaluate=med[0], stage_seconds=dict(G=med[1], CLIP=med[2], D=med[3]), timed_calls=len(calls), warmup_calls=1,
                thread_sweep_seconds_per_evaluate={str(n): round(v[0], 3) for n, v in sorted(sweep.items())},
                sample="oracle/ (torch-CPU fp32 restatement) on P=%d of the same workload (%d minibatch(es) of 4: one G call + one D "
                       "call each, models.py:108-129); torch intra-op threads swept over %s (one call each after a warm-up), best = %d "
                       "threads: median of %d call(s), %.2f s per _evaluate (G %.2f / CLIP %.2f / D %.2f)"
                       % (pop, pop // BATCH, sorted(sweep), best, len(calls), med[0], med[1], med[2], med[3]))


def bench_gpt2(args):
    """BASELINE.json configs[4] (not the headline): the GPT2 img2txt config through `GenerationProblem._evaluate` — the path run.py
    drives (problem.py:14-29 -> models.py:32-62 -> generator.py:52-59): GPT-2-small token-latent decode on the device (20 latent + 3
    prompt tokens, 30 greedy steps, gpt2/sample.py:21-36), `parse_out` (ids -> text, cut at <|endoftext|> / 50 characters) and
    `clip.tokenize` on the host, CLIP text tower + cosine against the image feature on the device; pop = 64, 1 GPU.  The reference's
    vocabulary FILES are not on the box: BPE assets of the real sizes (50257 / 49408 ids) in the reference's formats are generated
    (synth.write_bpe_assets), so the host stage is the real code on real-sized tables; its ms are reported separately."""
    import tempfile
    import types
    import torch
    assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback)"
    from clip_glass_amd import config as gconfig
    from clip_glass_amd import synth
    from clip_glass_amd.engine import device_info
    from clip_glass_amd.problem import GenerationProblem
    P = args.pop
    clipg = (768, 12, 12, 32, 224, 512)
    tmp = tempfile.mkdtemp(prefix="glass_bpe_")
    enc, voc, bpe = synth.write_bpe_assets(tmp)
    cfg = types.SimpleNamespace(config="GPT2", device="cuda:0", target="unused")
    vars(cfg).update(gconfig.get_config("GPT2"))
    vars(cfg).update(weights="synthetic:5", clip_weights="synthetic:0", clip_geometry=clipg, clip_text_geometry=dict(width=512, layers=12),
                     encoder=enc, vocab=voc, bpe_path=bpe, target_features=synth.normal(3, "imgfeat", (512,)), pop_size=P, max_pop=P)
    prob = GenerationProblem(cfg)
    gen = prob.generator
    eng = gen.engine
    assert len(gen.model.init_tokens) == 3, "the prompt must be 3 tokens (config.py:25 'the picture of')"
    # stage clocks around the product's own methods (wall, host side); the device decode reports its hipEvent time itself
    clock = dict(decode=0.0, parse=0.0, tokenize=0.0, text=0.0, dec_gpu_ms=0.0, tok_fail=0)

    def timed(obj, name, key, after=None):
        fn = getattr(obj, name)

        def wrap(*a, **k):
            t0 = time.perf_counter()
            r = fn(*a, **k)
            clock[key] += time.perf_counter() - t0
            if after:
                after()
            return r
        setattr(obj, name, wrap)
    timed(gen.model, "decode_tokens", "decode", after=lambda: clock.__setitem__("dec_gpu_ms", clock["dec_gpu_ms"] + eng.last_gpu_ms()))
    timed(gen.model, "parse_out", "parse")
    timed(eng, "encode_text", "text")
    tok_fn = gen.tokenizer.tokenize

    def tok_wrap(texts):
        t0 = time.perf_counter()
        try:
            return tok_fn(texts)
        except Exception:
            clock["tok_fail"] += 1          # generator.py:53-56: the whole population then scores 0 and the text tower is skipped
            raise
        finally:
            clock["tokenize"] += time.perf_counter() - t0
    gen.tokenizer.tokenize = tok_wrap

    def step(seed):
        x = np.random.RandomState(seed).randint(0, 50257, size=(P, 20))
        out = {}
        prob._evaluate(x, out)
        return out["F"]
    for s in range(max(args.warmup, 1)):
        step(s)
    torch.cuda.synchronize()
    for k in clock:
        clock[k] = 0 if k == "tok_fail" else 0.0
    t0 = time.perf_counter()
    for s in range(args.steps):
        F = step(100 + s)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert F.shape == (P,) and np.isfinite(F).all()
    assert clock["tok_fail"] == 0, "clip.tokenize refused a decoded text: the timed steps skipped the text tower"
    assert np.abs(F).max() > 0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, fitness=F)
    dec_ms = clock["dec_gpu_ms"]
    # decode = weight streaming: every fp32 weight of the 12 blocks + the tied lm_head is read once per step
    n_w = 12 * (768 * 2304 + 768 * 768 + 2 * 768 * 3072) + 50257 * 768
    bytes_per_decode = 4.0 * n_w * 30
    gbs = bytes_per_decode * args.steps / (dec_ms * 1e-3) / 1e9
    traffic, traffic_src = None, None
    tpath = os.path.join(ROOT, "profiles", "traffic_latest_gpt2.json")
    if os.path.exists(tpath):
        tj = json.load(open(tpath))
        traffic = tj.get("bytes_per_decode")
        traffic_src = tj.get("source")
    per = lambda k: clock[k] / args.steps * 1e3
    out = dict(metric="candidate token-latents scored/sec (GPT2 decode -> CLIP text score), GPT2 pop=%d" % P, value=P * args.steps / dt,
               unit="candidates/s", n_gpus=1, steps=args.steps, warmup=args.warmup, ms_per_step=dt / args.steps * 1e3, higher_is_better=True,
               scaling="weak", vs_baseline=None, dtype="f32", data="synthetic",
               config=dict(workload="GPT2: GenerationProblem._evaluate of the GPT2 img2txt config — GPT-2-small greedy decode (23-token "
                                    "context, 30 steps, fp32, KV cache, one hipGraph per single-token step), parse_out + clip.tokenize "
                                    "on the host (generated BPE tables of the real sizes, 50257 / 49408 ids), CLIP ViT-B/32 text tower "
                                    "+ cosine, pop=%d" % P, pop_per_gpu=P, device=device_info(0)["name"]),
               stage_ms=dict(decode_wall=per("decode"), decode_gpu=dec_ms / args.steps, parse_out_host=per("parse"),
                             clip_tokenize_host=per("tokenize"), text_tower_wall=per("text"),
                             other_host=(dt - clock["decode"] - clock["parse"] - clock["tokenize"] - clock["text"]) / args.steps * 1e3),
               gpu_active_s=dec_ms * 1e-3,      # device time of the decodes (hipEvents; the text tower's launches are not in it)
               roofline=dict(bound="hbm", kernel="gemm_f32_stream_kernel / gpt2_head_kernel (weight streaming, 30 steps)", achieved=gbs, peak=HBM_PEAK_GBS,
                             unit="GB/s", frac=gbs / HBM_PEAK_GBS, traffic=traffic, traffic_source=traffic_src,
                             decode_ms_per_population=dec_ms / args.steps, algorithmic_bytes_per_decode=bytes_per_decode))
    print(json.dumps(out))
    eng.close()
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)          # the generated BPE tables


def run_legs(args):
    """`bench.py --config biggan512` and `--config gpt2` as child processes (fresh engines, --leg-steps timed steps each); their one-line
    JSON results, trimmed to what identifies and prices the leg."""
    import subprocess
    legs = {}
    # the children must not inherit the parent's detail-dump path (the biggan512 leg would write its own table over the headline's;
    # ADVICE r4) — and a leg that hangs may cost the driver's line 4 minutes, not 10
    child_env = {k: v for k, v in os.environ.items() if k not in ("GLASS_BENCH_DETAIL", "GLASS_BENCH_UNIFORM_POP", "GLASS_BENCH_FULLPROF")}
    for name, extra in (("biggan512", ["--warmup", "2", "--no-cpu-baseline"]), ("gpt2", ["--warmup", "1"])):
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--config", name, "--steps", str(args.leg_steps), "--full", "--no-legs"] + extra,
                               capture_output=True, text=True, timeout=240, env=child_env)
            line = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
            if r.returncode != 0 or not line:
                legs[name] = dict(error=(r.stderr or r.stdout)[-400:], returncode=r.returncode)
                continue
            d = json.loads(line[-1])
            keep = ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "dtype", "data", "gpu_active_s", "stage_ms")
            leg = {k: d[k] for k in keep if k in d}
            leg["config"] = d["config"]
            rf = d.get("roofline", {})
            leg["roofline"] = {k: rf[k] for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "traffic_ratio", "launches", "avg_ms", "families",
                                                  "whole_pass_frac_of_mfma_peak", "whole_pass_tflops", "decode_ms_per_population",
                                                  "algorithmic_bytes_per_decode") if k in rf}
            leg["leg_wall_s"] = time.time() - t0
            legs[name] = leg
        except Exception as ex:       # a leg must never take the headline line down with it
            legs[name] = dict(error=repr(ex)[:400])
    return legs


def main():
    global BATCH
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50, help="timed _evaluate calls (the config runs 50 generations)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="ffhq", help="model size key (tests/models.py naming); ffhq = the headline")
    ap.add_argument("--pop", type=int, default=POP)
    ap.add_argument("--full", action="store_true", help="also measure the roofline / per-kernel table, the CPU baseline and the "
                                                         "biggan512 / gpt2 legs (a plain run times the headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's fitness rows to DIR/fitness.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline-pop", type=int, default=BATCH, help="candidates in the CPU baseline sample (multiple of 4; 64 = the whole headline population, ~4 min)")
    ap.add_argument("--cpu-baseline-budget", type=float, default=150.0, help="seconds the CPU baseline's sweep + fresh calls may spend (a P = 64 sweep needs ~1500)")
    ap.add_argument("--cpu-baseline-threads", type=int, default=0, help="torch intra-op threads of the CPU baseline (0 = sweep 8/16/32/64/128 and report the best)")
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--no-legs", action="store_true", help="with --full: skip the biggan512 / gpt2 legs attached to the line")
    ap.add_argument("--leg-steps", type=int, default=5)
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # launched bare as `python bench.py --gpus N`: become the launcher — one process per GPU under torch.distributed.run
        # (RCCL rendezvous on 127.0.0.1); rank 0's JSON line is the only thing on stdout
        import socket
        import subprocess
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        if os.environ.get("GLASS_BENCH_LAUNCH_DRYRUN"):      # CPU test hook: show the launch line, start nothing
            print(json.dumps(cmd))
            sys.exit(0)
        sys.exit(subprocess.call(cmd))

    if args.config == "gpt2":
        return bench_gpt2(args)

    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist = None
    json_fd = None
    if world > 1 or os.environ.get("GLASS_BENCH_FORCE_DIST"):   # torchrun path (RCCL); forced at world 1 for testing
        # RCCL prints a version banner on the C-level stdout at init; keep stdout to the ONE JSON line: fd 1 -> stderr for
        # everything else, the JSON goes to the saved descriptor
        sys.stdout.flush()
        json_fd = os.dup(1)
        os.dup2(2, 1)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if os.environ.get("GLASS_BENCH_SHARE_GPU"):      # test knob: several ranks on the one GPU of a test box
            local_rank = local_rank % max(torch.cuda.device_count(), 1)
        torch.cuda.set_device(local_rank)
        backend = os.environ.get("GLASS_BENCH_BACKEND", "nccl")    # "nccl" IS RCCL on ROCm; gloo only for the shared-GPU test
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        assert dist.get_world_size() == world
        if os.environ.get("GLASS_BENCH_FORCE_DIST") is None:
            assert world == args.gpus, "--gpus %d but the launcher started %d ranks" % (args.gpus, world)
    assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback)"
    torch.cuda.set_device(local_rank)

    from clip_glass_amd import synth
    from clip_glass_amd.engine import Engine, device_info
    from clip_glass_amd.parallel import ShardedEvaluator

    cfgs = {"ffhq": dict(channels=synth.FFHQ_CHANNELS, latent=512, mapping=8, clip=(768, 12, 12, 32, 224, 512)),
            "mid": dict(channels=[32, 64, 64, 64, 64], latent=64, mapping=3, clip=(128, 2, 2, 8, 32, 64)),
            # BASELINE.json configs[2] (not the headline): DeepMindBigGAN512 + CLIP ViT-B/32, batch_size 8 (config.py:66)
            "biggan512": dict(biggan=dict(layers=synth.BIGGAN_LAYERS[512], attention_pos=8, ch=128, z_dim=128, num_classes=1000),
                              clip=(768, 12, 12, 32, 224, 512))}
    cfg = cfgs[args.config]
    P = args.pop
    biggan = cfg.get("biggan")
    w, layers, heads, patch, res, emb = cfg["clip"]
    if biggan:
        BATCH = 8
        b = biggan
        sd = synth.make_biggan_state(synth.biggan_spec(b["layers"], b["attention_pos"], b["ch"], b["z_dim"], b["num_classes"]), 0)
        sd.update(synth.make_state(synth.clip_visual_spec(w, layers, patch, res, emb), 0))
        eng = Engine([], batch_size=BATCH, max_pop=P, chunk=args.chunk, clip=cfg["clip"], device=local_rank, biggan=biggan)
        n_obj = 1

        def population(seed, n):
            return synth.biggan_population(seed, n, b["z_dim"], b["num_classes"])
    else:
        sd = synth.make_state(synth.stylegan2_g_spec(cfg["channels"], cfg["latent"], cfg["mapping"]), 0)
        sd.update(synth.make_state(synth.stylegan2_d_spec(cfg["channels"]), 0))
        sd.update(synth.make_state(synth.clip_visual_spec(w, layers, patch, res, emb), 0))
        eng = Engine(cfg["channels"][::-1], latent_size=cfg["latent"], mapping_layers=cfg["mapping"], batch_size=BATCH,
                     use_discriminator=True, n_obj=2, max_pop=P, chunk=args.chunk, clip=cfg["clip"], noise_mode=1,
                     noise_seed=1234, device=local_rank)
        n_obj = 2

        def population(seed, n):
            return synth.latents(seed, n, cfg["latent"])
    eng.load_state(sd)
    eng.finalize()
    # synthetic target: a pass with a dummy target to get features, then sims in ~[0.5, 0.9]
    eng.set_target(np.ones(emb, np.float32))
    # (GLASS_BENCH_UNIFORM_POP: the PMC passes want every launch of the run at the full population — tools/measure_traffic.sh)
    P0 = P if os.environ.get("GLASS_BENCH_UNIFORM_POP") else BATCH
    eng.evaluate(population(999, P0))
    target = synth.make_target(eng.details(P0)["features"][:BATCH])
    eng.set_target(target)

    ev = ShardedEvaluator(eng, dist, rank, world, BATCH)

    def sync():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # warm-up passes are profiled per launch (every kernel): they pick the dominant kernel symbol;
    # the timed region then carries hipEvent pairs only around THAT kernel's launches, so the
    # event overhead (~7 % with every launch instrumented) stays out of `value`.
    # stream mode of the timed region: 2 = CLIP's image tower on a second stream next to the discriminator (the engine's default),
    # 1 = chunk pipelining (GLASS_OVERLAP=1), 0 = one stream.  Every fully instrumented pass runs on ONE stream.
    mode = 1 if os.environ.get("GLASS_OVERLAP") else (0 if os.environ.get("GLASS_NO_CLIP_OVERLAP") else 2)
    prof = {}
    if args.full:
        eng.set_overlap(0)
        eng.set_profiling(True)
        warm = {}
        for s in range(max(args.warmup, 1)):
            ev.evaluate_local(population(1000 * rank + s, P), generation=s)
            warm = {}
            for r in eng.profile():
                kern = kernel_family(r["name"])
                a = warm.setdefault(kern, 0.0)
                warm[kern] = a + r["total_ms"]
        full_prof = {r["name"]: dict(launches=r["launches"], total_ms=r["total_ms"], flops=r["flops"], bytes=r["bytes"])
                     for r in eng.profile()}
        dominant = max(warm.items(), key=lambda kv: kv[1])[0]
        if os.environ.get("GLASS_BENCH_NOPROF"):
            eng.set_profiling(False)
        elif not os.environ.get("GLASS_BENCH_FULLPROF"):
            eng.set_profile_filter(dominant)
        eng.set_overlap(mode)
        ev.evaluate_local(population(1000 * rank + 99, P), generation=99)     # (one un-timed pass in the timed region's stream mode)
        eng.profile()
    else:
        # plain run: the warm-up passes already run in the timed region's stream mode, and no launch is instrumented
        eng.set_overlap(mode)
        for s in range(max(args.warmup, 1)):
            ev.evaluate_local(population(1000 * rank + s, P), generation=s)
    # the K fresh populations are drawn BEFORE the clock starts: drawing synthetic latents (numpy RandomState, ~1-2 ms of host time per
    # 64 x 512 population) is input synthesis, not the hot path — the timed region starts with its inputs ready in host memory and
    # still carries every H2D copy of them (the boundary takes host buffers, include/glass.h)
    pops = [population(1000 * rank + 100 + s, P) for s in range(args.steps)]
    sync()
    t0 = time.perf_counter()
    gpu_ms = 0.0
    for s in range(args.steps):
        F_all = ev.evaluate_local(pops[s], generation=100 + s)
        gpu_ms += eng.last_gpu_ms()         # hipEvent pair around the whole pass on the engine's main stream (engine.cpp run_pass)
        if args.full:
            for r in eng.profile():
                a = prof.setdefault(r["name"], dict(launches=0, total_ms=0.0, flops=0.0, bytes=0.0))
                for k in a:
                    a[k] += r[k]
    sync()
    dt = time.perf_counter() - t0
    if args.full:
        eng.set_profiling(False)
        # one extra pass OUTSIDE the timed region, single stream + every launch instrumented: clean per-kernel
        # durations (in the timed region kernels of the two streams co-run and stretch each other)
        eng.set_overlap(0)
        eng.set_profile_filter("")
        eng.set_profiling(True)
        ev.evaluate_local(population(1000 * rank + 500, P), generation=500)
        iso = {}
        for r in eng.profile():
            kk = r["name"].split("@")[1] if "@" in r["name"] else r["name"]
            a3 = iso.setdefault(kk, dict(launches=0, total_ms=0.0, flops=0.0, bytes=0.0))
            for k3 in a3:
                a3[k3] += r[k3]
        eng.set_profiling(False)
    if dist is not None:
        tt = torch.tensor([dt], device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    assert F_all.shape == (P * world, n_obj) and np.isfinite(F_all).all()

    if rank == 0:
        if args.full:
            # dominant kernel = the SOURCE kernel (all its template instances) with the largest share of device time
            iso_fam = {}
            for k3, v3 in iso.items():
                a4 = iso_fam.setdefault(k3.split("<")[0], dict(launches=0, total_ms=0.0, flops=0.0, bytes=0.0))
                for k4 in a4:
                    a4[k4] += v3[k4]
            by_kernel = {}
            for name, a in prof.items():
                kern = kernel_family(name)
                b = by_kernel.setdefault(kern, dict(launches=0, total_ms=0.0, flops=0.0, bytes=0.0))
                for k in b:
                    b[k] += a[k]
            if not by_kernel:
                by_kernel = {"(profiling off)": dict(launches=0, total_ms=0.0, flops=0.0, bytes=0.0)}
            kern, a = max(by_kernel.items(), key=lambda kv: kv[1]["total_ms"])
            secs = a["total_ms"] * 1e-3
            tf = a["flops"] / secs / 1e12 if secs > 0 else 0.0          # algorithmic FLOP of its launches / their duration
            gbs = a["bytes"] / secs / 1e9 if secs > 0 else 0.0          # algorithmic bytes (in + out maps + weights)
            warm_total = sum(warm.values())
            total_ms = sum(v["total_ms"] for v in full_prof.values())
            total_flops = sum(v["flops"] for v in full_prof.values())
            # the roof that binds = the one the kernel sits closer to (the same kernel runs
            # MFMA-bound mid-resolution layers and HBM-bound 512^2/1024^2 layers)
            frac_mfma, frac_hbm = tf / MFMA_PEAK_TFLOPS, gbs / HBM_PEAK_GBS
            # `traffic`: NOT measured in this run — the counters need their own rocprofv3 --pmc passes (tools/measure_traffic.sh: one
            # FETCH_SIZE and one WRITE_SIZE pass of this same command, every launch at the full population); the stored table is
            # profiles/traffic_latest.json and the line says so
            traffic, traffic_src = None, None
            tname = "traffic_latest_biggan512.json" if biggan else "traffic_latest.json"
            tpath = os.path.join(ROOT, "profiles", tname)
            traffic_rows = json.load(open(tpath)).get("per_kernel", {}) if os.path.exists(tpath) else {}
            if traffic_rows:
                row = match_family(kern, traffic_rows)
                if row:
                    traffic = row["bytes_per_launch"]
                    traffic_src = ("stored rocprofv3 --pmc passes (FETCH_SIZE x 2 + WRITE_SIZE, tools/measure_traffic.sh -> profiles/%s), "
                                   "average over this kernel's %d launches at P = %d; not collected by this run" % (tname, row["launches"], P))
            if frac_hbm > frac_mfma:
                roofline = dict(bound="hbm", achieved=gbs, peak=HBM_PEAK_GBS, unit="GB/s", frac=frac_hbm)
            else:
                roofline = dict(bound="mfma", achieved=tf, peak=MFMA_PEAK_TFLOPS, unit="TFLOP/s", frac=frac_mfma)
            alg_bpl = a["bytes"] / max(a["launches"], 1)
            roofline.update(kernel=kern, launches=a["launches"], avg_ms=a["total_ms"] / max(a["launches"], 1), traffic=traffic,
                            traffic_source=traffic_src, traffic_ratio=(traffic / alg_bpl if traffic and alg_bpl else None),
                            algorithmic_tflops=tf, algorithmic_gbs=gbs, frac_of_mfma_peak=frac_mfma, frac_of_hbm_peak=frac_hbm,
                            algorithmic_bytes_per_launch=a["bytes"] / max(a["launches"], 1),
                            algorithmic_flop_per_launch=a["flops"] / max(a["launches"], 1),
                            share_of_gpu_time=warm.get(kern, 0.0) / warm_total if warm_total else None,
                            instances=sorted(k for k in iso if k.split("<")[0] == kern),
                            isolated=(dict(avg_ms=iso_fam[kern]["total_ms"] / max(iso_fam[kern]["launches"], 1),
                                           algorithmic_tflops=iso_fam[kern]["flops"] / (iso_fam[kern]["total_ms"] * 1e-3) / 1e12,
                                           algorithmic_gbs=iso_fam[kern]["bytes"] / (iso_fam[kern]["total_ms"] * 1e-3) / 1e9,
                                           note="same kernel, one extra single-stream pass after the timed region")
                                      if kern in iso_fam and iso_fam[kern]["total_ms"] > 0 else None),
                            concurrency={0: "single stream",
                                         1: "two HIP streams (GLASS_OVERLAP=1): durations include co-running kernels",
                                         2: "G and D on one stream; CLIP's image tower on a second stream next to D (G launches never "
                                            "have a co-runner, D launches may; `isolated` = one-stream pass)"}[mode],
                            # whole pass: algorithmic FLOP of one population (the reference's op count: every launch's tag) over the
                            # TIMED region's ms_per_step (driver-comparable) — and over the instrumented one-stream pass for reference
                            whole_pass_tflops=total_flops / (dt / args.steps) / 1e12,
                            whole_pass_frac_of_mfma_peak=total_flops / (dt / args.steps) / 1e12 / MFMA_PEAK_TFLOPS,
                            whole_pass_algorithmic_gflop_per_candidate=total_flops / P / 1e9,
                            families=family_table(iso, dt / args.steps * 1e3, traffic_rows),
                            instrumented_pass_ms=total_ms,
                            instrumented_pass_frac_of_mfma_peak=(total_flops / (total_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS) if total_ms else None)
        if biggan:
            metric = "candidate latents scored/sec (GAN→CLIP fitness), DeepMindBigGAN512 pop=%d" % P
            workload = ("DeepMindBigGAN512: BigGAN-deep 512px G + CLIP ViT-B/32, pop=%d per GPU, batch_size=%d, n_obj=1" % (P, BATCH))
        else:
            metric = METRIC
            workload = ("StyleGAN2_ffhq_d: StyleGAN2 config-f %dpx G+D + CLIP ViT-B/32, pop=%d per GPU, batch_size=%d, n_obj=2"
                        % (4 << (len(cfg["channels"]) - 1), P, BATCH))
        out = dict(metric=metric, value=P * world * args.steps / dt, unit="candidates/s", n_gpus=(dist.get_world_size() if dist is not None else 1),
                   steps=args.steps, warmup=args.warmup, ms_per_step=dt / args.steps * 1e3, higher_is_better=True,
                   scaling="weak", vs_baseline=None, dtype="f16", data="synthetic",
                   config=dict(workload=workload, pop_per_gpu=P, global_pop=P * world, batch_size=BATCH, parallelism="population-shard x%d" % world,
                               device="%(name)s, %(cus)d CUs" % device_info(local_rank), hbm_gib=round(device_info(local_rank)["hbm_bytes"] / 2 ** 30)),
                   # device time of the timed region = sum over its steps of the hipEvent interval around each pass (H2D of the latents
                   # ... D2H of F): checkable against `ms_per_step` even when an smi sampler misses the ~1 s window
                   gpu_active_s=gpu_ms * 1e-3, gpu_active_frac_of_timed_region=gpu_ms * 1e-3 / dt)
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, fitness=F_all)
        if args.full:
            out["roofline"] = roofline
            if world == 1 and not args.no_cpu_baseline and not biggan:
                out["cpu_baseline"] = cpu_baseline(sd, cfg, target, pop=max(BATCH, args.cpu_baseline_pop // BATCH * BATCH), budget_s=args.cpu_baseline_budget,
                                                   threads=((args.cpu_baseline_threads,) if args.cpu_baseline_threads else (8, 16, 32, 64, 128)))
            if world == 1 and args.config == "ffhq" and not args.no_legs and dist is None:
                # the other single-GPU configs of BASELINE.json (configs[2] DeepMindBigGAN512, configs[4] GPT2) as short legs of the
                # same driver-run line, each with its own roofline; the headline engine is closed first
                eng.close()
                out["legs"] = run_legs(args)
            if os.environ.get("GLASS_BENCH_DETAIL"):
                with open(os.environ["GLASS_BENCH_DETAIL"], "w") as f:
                    wk = {}
                    for name, a2 in full_prof.items():
                        kk = name.split("@")[1] if "@" in name else name
                        b2 = wk.setdefault(kk, dict(launches=0, total_ms=0.0, flops=0.0, bytes=0.0))
                        for k2 in b2:
                            b2[k2] += a2[k2]
                    json.dump(dict(per_tag=full_prof, per_kernel=wk, seconds=dt / args.steps, note="per_tag/per_kernel: ONE fully "
                                   "instrumented warm-up pass; timed region instruments only the dominant kernel"), f, indent=1)
        if json_fd is not None:
            os.write(json_fd, (json.dumps(out) + "\n").encode())
        else:
            print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
