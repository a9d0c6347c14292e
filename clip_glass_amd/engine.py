"""ctypes binding of libglass.so (include/glass.h) — the drop-in boundary.

The library is built in-tree by `__graft_entry__.build()` / `make -C clip_glass_amd/csrc`.
There is NO CPU fallback: if the shared library is missing or the HIP device is
absent, construction raises (the reference would `sys.exit(1)` on missing weights,
models.py:18-20,93-101; here errors surface as RuntimeError with glass_last_error()).

The C side of every function is one entry of SIGNATURES (RESTYPES where it does not return int) and the three structs are mirrored once;
tests/test_engine_signatures.py holds all of it against the header's text.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libglass.so")
MAX_BLOCKS = 12
MAX_BG_LAYERS = 16
GEN_STYLEGAN2, GEN_BIGGAN_DEEP = 0, 1


class GlassConfig(C.Structure):
    """glass_config, every field in header order.  Each feature appended its fields last and zero means off, so a library built before a
    field (an A/B build loaded through GLASS_LIB) reads a prefix of this struct."""
    _fields_ = [("device", C.c_int32), ("n_blocks", C.c_int32), ("channels", C.c_int32 * MAX_BLOCKS),
                ("latent_size", C.c_int32), ("mapping_layers", C.c_int32), ("batch_size", C.c_int32),
                ("mbstd_group", C.c_int32), ("use_discriminator", C.c_int32), ("n_obj", C.c_int32),
                ("max_pop", C.c_int32), ("chunk", C.c_int32),
                ("clip_width", C.c_int32), ("clip_layers", C.c_int32), ("clip_heads", C.c_int32),
                ("clip_patch", C.c_int32), ("clip_res", C.c_int32), ("clip_embed", C.c_int32),
                ("noise_mode", C.c_int32), ("noise_seed", C.c_uint64),
                ("generator", C.c_int32), ("bg_ch", C.c_int32), ("bg_z_dim", C.c_int32), ("bg_num_classes", C.c_int32),
                ("bg_n_layers", C.c_int32), ("bg_layers", (C.c_int32 * 3) * MAX_BG_LAYERS),
                ("bg_attention_pos", C.c_int32), ("bg_n_stats", C.c_int32), ("bg_eps", C.c_float),
                ("bg_truncation", C.c_float),
                ("clip_resize", C.c_int32), ("clip_normalize", C.c_int32),
                ("clip_arch", C.c_int32), ("clip_rn_layers", C.c_int32 * 4),
                ("lpips_size", C.c_int32), ("lpips_lambda", C.c_float),
                ("sim_columns", C.c_int32),
                ("anchor", C.c_int32), ("anchor_lambda", C.c_float)]


PROMPT_MODES = {"sum": 0, "pareto": 1}      # include/glass.h "Prompt sets"
PROMPT_MAX = 16


class GlassNoise(C.Structure):
    _fields_ = [("n_minibatches", C.c_int32), ("n_layers", C.c_int32),
                ("planes", C.POINTER(C.POINTER(C.c_float)))]


class ProfRow(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("launches", C.c_int64), ("total_ms", C.c_double),
                ("flops", C.c_double), ("bytes", C.c_double)]


# The C signature of every function of include/glass.h, argument by argument, in header order.  glass_engine* is an opaque handle (h);
# load_library() applies the table once; tests/test_engine_signatures.py holds it, RESTYPES and the three structs against the header.
i32, i64, u64, f32, f64, h, cp = C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double, C.c_void_p, C.c_char_p
fp, ip, lp, dp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
SIGNATURES = {
    "glass_last_error": [],
    "glass_version": [],
    "glass_clip_geometry_supported": [i32] * 6,
    "glass_clip_resnet_supported": [ip, i32, i32, i32],
    "glass_clip_preprocess_supported": [i32] * 4,
    "glass_clip_views_supported": [i32] * 6,
    "glass_host_clip_view_boxes": [u64, i32, i32, i32, i32, i32, i32, ip],
    "glass_lpips_supported": [i32, i32],
    "glass_prompt_set_supported": [i32, i32, i32],
    "glass_engine_set_targets": [h, fp, fp, i32, i32, i32],
    "glass_engine_last_set_details": [h, i32, fp],
    "glass_engine_encode_generated": [h, fp, i32, fp],
    "glass_edit_supported": [i32, i32, i32, i32, i32, i32, f32, i32],
    "glass_engine_set_anchor": [h, fp],
    "glass_engine_last_anchor": [h, i32, fp],
    "glass_engine_set_direction_source": [h, fp],
    "glass_engine_last_direction_source": [h, fp],
    "glass_engine_create": [C.POINTER(GlassConfig), C.POINTER(h)],
    "glass_engine_set_lpips_target": [h, fp, i32],
    "glass_engine_lpips": [h, fp, fp, i32, fp],
    "glass_engine_last_lpips": [h, i32, fp],
    "glass_engine_set_clip_views": [h, i32, i32, i32, i32],
    "glass_engine_destroy": [h],
    "glass_host_layer_psi": [i32, f32, i32, fp],
    "glass_engine_set_latent_space": [h, i32],
    "glass_engine_set_truncation": [h, f32, i32],
    "glass_engine_latent_row": [h, ip, ip],
    "glass_engine_map_latents": [h, fp, i32, fp],
    "glass_subspace_supported": [i32, i32, i32, i32, ip, cp, i32],
    "glass_engine_set_subspace_shape": [h, i32, i32],
    "glass_engine_set_subspace": [h, ip, fp, fp],
    "glass_engine_expand_latents": [h, fp, i32, fp],
    "glass_engine_load_tensor": [h, cp, fp, i32, lp],
    "glass_engine_finalize": [h],
    "glass_engine_set_target": [h, fp, i32],
    "glass_engine_encode_text": [h, ip, i32, i32, fp],
    "glass_engine_encode_image": [h, fp, i32, fp],
    "glass_engine_gpt2_decode": [h, ip, i32, i32, i32, ip],
    "glass_engine_gpt2_sample": [h, ip, i32, i32, i32, f32, i32, u64, i32, i32, i32, ip],
    "glass_engine_evaluate": [h, fp, i32, i32, i32, C.POINTER(GlassNoise), fp],
    "glass_engine_last_details": [h, i32, fp, fp, fp],
    "glass_engine_last_view_details": [h, i32, fp, fp, ip],
    "glass_engine_generate": [h, fp, i32, i32, i32, C.POINTER(GlassNoise), fp],
    "glass_engine_last_gpu_ms": [h, fp],
    "glass_engine_last_F_device": [h, i32, C.POINTER(C.c_void_p)],
    "glass_engine_set_profiling": [h, i32],
    "glass_engine_set_profile_filter": [h, cp],
    "glass_engine_get_profile": [h, C.POINTER(ProfRow), i32, ip],
    "glass_engine_set_overlap": [h, i32],
    "glass_engine_set_biggan_tap": [h, i32],
    "glass_engine_get_biggan_tap": [h, fp, i64, ip],
    "glass_search_supported": [i32] * 4,
    "glass_engine_set_search": [h, i32, i32, f64, f64, f64, f64, f64, u64],
    "glass_engine_set_search_operators": [h, f64, f64, f64, f64, f64, u64],
    "glass_search_mixed_supported": [i32] * 5,
    "glass_engine_set_search_mixed": [h, i32, i32, i32, f64, f64, f64, f64, f64, f64, f64, u64],
    "glass_engine_set_search_operators_mixed": [h, f64, f64, f64, f64, f64, f64, f64, u64],
    "glass_engine_search_init": [h, fp],
    "glass_engine_search_vary": [h, i32],
    "glass_engine_search_evaluate": [h, i32, i32, i32],
    "glass_engine_search_survive": [h, i32],
    "glass_engine_search_step": [h, i32],
    "glass_engine_search_read": [h, fp, fp, ip, dp, fp, fp, ip, ip],
    "glass_engine_latent_uploads": [h, lp, lp],
    "glass_search_islands_supported": [i32] * 7,
    "glass_engine_set_search_islands": [h, i32, i32, i32],
    "glass_engine_set_island_weights": [h, fp, i32, i32],
    "glass_engine_search_migrate": [h, i32],
    "glass_engine_search_read_islands": [h, ip],
    "glass_engine_search_init_cma": [h, dp, dp, f64],
    "glass_engine_search_read_cma": [h, dp, dp, dp, dp, dp, ip, fp, fp],
    "glass_device_info": [i32, cp, i32, ip, lp],
}
RESTYPES = {"glass_last_error": cp, "glass_version": cp, "glass_engine_destroy": None}      # every other function returns int


def bind(lib, signatures, restypes={}):
    """Give every function of the table that `lib` exports its C signature.  A name the build lacks is skipped: an older build of
    libglass.so loaded through GLASS_LIB (the A/B knob) predates the newer functions, and calling one of those fails by name."""
    for name, argtypes in signatures.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argtypes, restypes.get(name, C.c_int)


_lib = None


def load_library(path=None):
    """Load libglass.so; raises OSError/RuntimeError loudly when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("GLASS_LIB") or LIB_PATH      # GLASS_LIB: A/B knob (a second build of libglass.so on the same box)
    if not os.path.exists(path):
        raise RuntimeError("libglass.so not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "or `make -C clip_glass_amd/csrc` — there is no CPU fallback" % path)
    lib = C.CDLL(path)
    bind(lib, SIGNATURES, RESTYPES)
    _lib = lib
    return lib


def _check(lib, rc):
    if rc != 0:
        raise RuntimeError("libglass error %d: %s" % (rc, lib.glass_last_error().decode()))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _verdict(rule, *args):
    """(True, "") or (False, glass_last_error()) from glass_<rule>_supported(*args): the library's own rules, host only."""
    lib = load_library()
    rc = getattr(lib, "glass_%s_supported" % rule)(*args)
    return (True, "") if rc == 0 else (False, lib.glass_last_error().decode())


def clip_geometry_supported(geometry):
    """(ok, message) for a CLIP image tower (width, layers, heads, patch, input_res, embed): the library's own rule, the one
    glass_engine_create applies.  Host only: needs the built library, not a GPU."""
    return _verdict("clip_geometry", *[int(v) for v in geometry])


def clip_preprocess_supported(gen_res, clip_res, clip_resize, clip_normalize):
    """(ok, message) for the CLIP preprocessing fields (clip_resize, clip_normalize) from a gen_res px image to clip_res: the library's
    own rule, the one glass_engine_create applies.  Host only."""
    return _verdict("clip_preprocess", int(gen_res), int(clip_res), int(clip_resize), int(clip_normalize))


def clip_resnet_supported(geometry):
    """(ok, message) for a CLIP ResNet image tower (layers4, width, input_res, embed): the library's own rule, the one
    glass_engine_create applies.  Host only: needs the built library, not a GPU."""
    layers, width, res, embed = geometry
    if len(layers) != 4:
        return False, "unsupported CLIP ResNet geometry: layers must hold four stage depths, got %r" % (tuple(layers),)
    return _verdict("clip_resnet", (C.c_int32 * 4)(*[int(v) for v in layers]), int(width), int(res), int(embed))


def lpips_supported(gen_res, lpips_size):
    """(ok, message) for the perceptual objective at VGG input side lpips_size on a gen_res px generator (0: the side alone): the
    library's own rule, the one glass_engine_create applies.  Host only."""
    return _verdict("lpips", int(gen_res), int(lpips_size))


def lpips_n_obj(use_discriminator, lpips_lambda):
    """Columns of F with the perceptual objective on (include/glass.h): -sim, the hinge with D, and the distance unless lambda folds it in."""
    return 1 + int(bool(use_discriminator)) + int(float(lpips_lambda) == 0.0)


def prompt_mode_id(mode):
    """The ABI's mode of a prompt set: "sum" -> 0, "pareto" -> 1 (ints pass through); ValueError lists the names otherwise."""
    if mode in PROMPT_MODES:
        return PROMPT_MODES[mode]
    if isinstance(mode, (int, np.integer)) and not isinstance(mode, bool):
        return int(mode)
    raise ValueError("unknown prompt_mode %r: expected one of %s" % (mode, ", ".join(PROMPT_MODES)))


def prompt_set_supported(n_entries, mode="sum", sim_columns=0):
    """(ok, message) for a prompt set of n_entries in `mode` on an engine with `sim_columns`: the library's own rule, the one
    glass_engine_set_targets applies.  Host only."""
    return _verdict("prompt_set", int(n_entries), prompt_mode_id(mode), int(sim_columns))


def prompt_n_obj(sim_columns, use_discriminator, lpips_column=False):
    """Columns of F on an engine with `sim_columns` similarity columns (include/glass.h): those, the hinge with D, the LPIPS distance when
    it is its own column."""
    return max(int(sim_columns), 1) + int(bool(use_discriminator)) + int(bool(lpips_column))


def edit_n_obj(sim_columns, use_discriminator, lpips_column=False, anchor=False, anchor_lambda=0.0):
    """Columns of F with the latent anchor (include/glass.h "Image editing"): prompt_n_obj's, and the anchor distance when it is its own
    column (anchor on, anchor_lambda 0)."""
    return prompt_n_obj(sim_columns, use_discriminator, lpips_column) + int(bool(anchor) and float(anchor_lambda) == 0.0)


def edit_supported(generator="stylegan2", n_blocks=9, sim_columns=0, use_discriminator=False, lpips_column=False, anchor=False, anchor_lambda=0.0,
                   n_obj=1):
    """(ok, message) for the latent anchor's fields on an engine of that kind ("stylegan2", "biggan", or None: no generator — n_blocks is
    then taken as 0): the library's own rule (glass_edit_supported), the one glass_engine_create applies.  Host only."""
    gen = GEN_BIGGAN_DEEP if generator == "biggan" else GEN_STYLEGAN2
    nb = int(n_blocks) if generator == "stylegan2" else 0
    return _verdict("edit", gen, nb, int(sim_columns), int(bool(use_discriminator)), int(bool(lpips_column)), int(anchor), float(anchor_lambda),
                    int(n_obj))


def clip_view_permille(fraction):
    """The smallest crop side as the library takes it: per mille of the image side."""
    return int(round(1000 * float(fraction)))


def clip_views_tower_rows(clip=None, clip_resnet=None):
    """(tokens, width) of an image tower as glass_clip_views_supported counts them: a ViT's (res / patch)^2 + 1 tokens and its width; a ResNet
    tower's (res / 4)^2 positions of layer1 and its stem width."""
    if clip_resnet is not None:
        _, width, res, _ = clip_resnet
        return (int(res) // 4) ** 2, int(width)
    width, _, _, patch, res, _ = clip
    return (int(res) // int(patch)) ** 2 + 1, int(width)


def clip_views_supported(max_pop, tokens, width, clip_resize, views, min_permille):
    """(ok, message) for crop views over a tower of `tokens` rows x `width` per image (clip_views_tower_rows): the library's own rule, the
    one glass_engine_set_clip_views applies.  Host only."""
    return _verdict("clip_views", int(max_pop), int(tokens), int(width), int(clip_resize), int(views), int(min_permille))


def host_clip_view_boxes(seed, generation, views, gen_res, min_permille, flip, fixed):
    """int32 [views, 4] = (x0, y0, s, flip): the library's own boxes of a pass (glass_host_clip_view_boxes; numpy mirror:
    synth.clip_view_boxes).  Host only."""
    lib = load_library()
    out = np.empty((int(views), 4), dtype=np.int32)
    _check(lib, lib.glass_host_clip_view_boxes(int(seed) & 0xFFFFFFFFFFFFFFFF, int(generation), int(views), int(gen_res), int(min_permille),
                                               int(bool(flip)), int(bool(fixed)), out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


SEARCH_ALGORITHMS = {"ga": 0, "nsga2": 1, "cmaes": 2}     # GLASS_SEARCH_GA / _NSGA2 / _CMAES
SEARCH_MAX_POP = 1024
CMA_MIN_POP = 4


def search_supported(pop, n_var, n_obj, algorithm):
    """(ok, message) for a device search of `pop` rows of n_var variables with n_obj objectives under "ga" / "nsga2" / "cmaes": the library's own rule
    (glass_search_supported), the one glass_engine_set_search and finalize apply.  Host only."""
    if algorithm not in SEARCH_ALGORITHMS:
        return False, "device search: unknown algorithm %r (expected one of %s)" % (algorithm, ", ".join(SEARCH_ALGORITHMS))
    return _verdict("search", int(pop), int(n_var), int(n_obj), SEARCH_ALGORITHMS[algorithm])


SEARCH_MAX_ISLANDS = 64


def search_islands_supported(islands, pop, n_var, n_obj, algorithm, migrate_every=0, migrants=1):
    """(ok, message) for `islands` populations of `pop` rows each with ring migration of `migrants` rows every `migrate_every` generations
    (0: never): the library's own rule (glass_search_islands_supported), the one glass_engine_set_search_islands and finalize apply.  Host
    only."""
    if algorithm not in SEARCH_ALGORITHMS:
        return False, "device search: unknown algorithm %r (expected one of %s)" % (algorithm, ", ".join(SEARCH_ALGORITHMS))
    return _verdict("search_islands", int(islands), int(pop), int(n_var), int(n_obj), SEARCH_ALGORITHMS[algorithm], int(migrate_every),
                    int(migrants))


SEARCH_MAX_BITS = 4096


def mixed_search_supported(pop, n_real, n_bits, n_obj, algorithm):
    """(ok, message) for a device search of `pop` mixed rows — n_real real columns, then n_bits bit columns: the library's own rule
    (glass_search_mixed_supported), the one glass_engine_set_search_mixed and finalize apply.  Host only."""
    if algorithm not in SEARCH_ALGORITHMS:
        return False, "device search: unknown algorithm %r (expected one of %s)" % (algorithm, ", ".join(SEARCH_ALGORITHMS))
    return _verdict("search_mixed", int(pop), int(n_real), int(n_bits), int(n_obj), SEARCH_ALGORITHMS[algorithm])


LATENT_SPACES = {"z": 0, "w": 1, "w+": 2, "sub": 3}     # GLASS_LATENT_Z / _W / _WPLUS / _SUB
SUBSPACE_MAX_COMPONENTS = 512


def subspace_supported(n_lat, latent_size, groups, components, layer_group=None):
    """(ok, message) for latent space "sub" with `groups` groups of style layers and `components` directions on a generator of n_lat style
    layers (layer_group: int [n_lat], -1 = frozen; None checks the shape alone): the library's own rule (glass_subspace_supported), the one
    set_subspace_shape and set_subspace apply.  Host only."""
    lib = load_library()
    lg = None
    if layer_group is not None:
        lg = np.ascontiguousarray(layer_group, dtype=np.int32).reshape(-1)
        if lg.size != int(n_lat):
            return False, "subspace: layer_group must hold n_lat = %d values, got %d" % (int(n_lat), lg.size)
    why = C.create_string_buffer(512)
    rc = lib.glass_subspace_supported(int(n_lat), int(latent_size), int(groups), int(components),
                                      lg.ctypes.data_as(C.POINTER(C.c_int32)) if lg is not None else None, why, len(why))
    return (True, "") if rc == 0 else (False, why.value.decode())


def latent_space_id(name):
    """GLASS_LATENT_* of a latent space's name; ValueError lists the names otherwise."""
    if name not in LATENT_SPACES:
        raise ValueError("unknown latent_space %r: expected one of %s" % (name, ", ".join(LATENT_SPACES)))
    return LATENT_SPACES[name]


def truncation_cutoff_arg(cutoff):
    """None (every layer, as the reference's set_truncation takes it) -> the ABI's -1."""
    return -1 if cutoff is None else int(cutoff)


def host_layer_psi(n_lat, psi, cutoff=None):
    """float32 [n_lat]: the per-layer psi of the truncation trick (glass_host_layer_psi: the rule the setter and the pass use).  Host only;
    RuntimeError with the library's reason for a psi outside [0, 1] or a cutoff outside [-1, n_lat]."""
    lib = load_library()
    out = np.empty((max(int(n_lat), 1),), dtype=np.float32)
    _check(lib, lib.glass_host_layer_psi(int(n_lat), float(psi), truncation_cutoff_arg(cutoff), _fp(out)))
    return out


def device_info(device=0):
    lib = load_library()
    name = C.create_string_buffer(256)
    cus = C.c_int32()
    mem = C.c_int64()
    _check(lib, lib.glass_device_info(device, name, 256, C.byref(cus), C.byref(mem)))
    return dict(name=name.value.decode(), cus=cus.value, hbm_bytes=mem.value)


class Engine:
    """One engine per (process, GPU).  Not thread-safe; evaluate() is blocking."""

    def __init__(self, channels, latent_size=512, mapping_layers=8, batch_size=4, use_discriminator=True,
                 n_obj=2, max_pop=64, chunk=0, clip=(768, 12, 12, 32, 224, 512), noise_mode=1, noise_seed=0,
                 mbstd_group=4, device=0, biggan=None, clip_resize=0, clip_normalize=0, clip_resnet=None,
                 clip_views=0, clip_view_min=0.5, clip_view_flip=True, clip_view_fixed=False,
                 latent_space="z", truncation_psi=1.0, truncation_cutoff=None, lpips_size=0, lpips_lambda=0.0, sim_columns=0,
                 anchor=False, anchor_lambda=0.0, subspace_shape=None):
        """`biggan` = dict(layers=[(up, in_mult, out_mult), ...], attention_pos, ch, z_dim, num_classes, n_stats, eps,
        truncation) selects the BigGAN-deep generator (channels must then be empty, no discriminator).
        clip_resize / clip_normalize: how a generated image is prepared for CLIP (include/glass.h); (0, 0) is the reference's way.
        clip_resnet = (layers4, width, res, embed) selects CLIP's ModifiedResNet image tower (RN50: ((3, 4, 6, 3), 64, 224, 1024));
        `clip` is ignored then.
        clip_views = V >= 1 scores a candidate as the mean similarity over V crop views of its image (include/glass.h: view 0 is the whole
        image, the others random boxes at least clip_view_min of the side, mirrored at random unless clip_view_flip is False, redrawn
        every generation unless clip_view_fixed); 0 (default) is the reference's single whole-image score.
        latent_space "z" (default) / "w" / "w+" and truncation_psi / truncation_cutoff (StyleGAN2 only; include/glass.h): what a row of
        evaluate / generate is, and the truncation trick applied to it.  The defaults call neither setter: the reference's raw generator
        on z.  A psi or cutoff given here is set before finalize, which then keeps the per-layer buffer a later set_truncation with a
        cutoff needs.
        lpips_size = S > 0 turns the perceptual objective on (include/glass.h): the LPIPS-VGG16 distance between a candidate's image,
        area-downscaled to S px, and the image given to set_lpips_target().  lpips_lambda = 0: the distance is one more, last, column
        of F and n_obj must count it (lpips_n_obj); > 0: F[:, 0] = -sim + lambda * d and n_obj stays.  Needs the "lpips.*" tensors.
        sim_columns = K in [2, 4] makes an engine for a pareto prompt set (include/glass.h "Prompt sets"): K similarity columns, one per
        entry of set_targets(..., mode="pareto"), and n_obj must be prompt_n_obj(K, ...); 0 (default): the one similarity column.
        anchor = True turns the latent anchor on (include/glass.h "Image editing"; StyleGAN2 only): the mean squared distance between a
        candidate's dlatents and those of the row given to set_anchor().  anchor_lambda = 0: one more, last, column of F and n_obj must
        count it (edit_n_obj); > 0: F[:, 0] += anchor_lambda * d and n_obj stays.
        latent_space "sub" with subspace_shape = (G, K) (include/glass.h "Subspace latent space"): a row is G * K coefficients of K
        directions of W for each of G groups of style layers; set_subspace(layer_group, basis, base) after finalize() gives the directions."""
        self.lib = load_library()
        cfg = GlassConfig()
        cfg.anchor, cfg.anchor_lambda = int(bool(anchor)), float(anchor_lambda)
        cfg.sim_columns = int(sim_columns)
        cfg.lpips_size, cfg.lpips_lambda = int(lpips_size), float(lpips_lambda)
        cfg.device = device
        if biggan is not None:
            layers = list(biggan["layers"])
            cfg.generator = GEN_BIGGAN_DEEP
            cfg.bg_ch, cfg.bg_z_dim = int(biggan.get("ch", 128)), int(biggan.get("z_dim", 128))
            cfg.bg_num_classes = int(biggan.get("num_classes", 1000))
            cfg.bg_n_layers = len(layers)
            for i, (up, a, b) in enumerate(layers):
                cfg.bg_layers[i][0], cfg.bg_layers[i][1], cfg.bg_layers[i][2] = int(up), int(a), int(b)
            cfg.bg_attention_pos = int(biggan.get("attention_pos", 8))
            cfg.bg_n_stats, cfg.bg_eps = int(biggan.get("n_stats", 51)), float(biggan.get("eps", 1e-4))
            cfg.bg_truncation = float(biggan.get("truncation", 1.0))
            latent_size = cfg.bg_z_dim + cfg.bg_num_classes
            channels, use_discriminator, noise_mode = [], False, 0
            n_obj = lpips_n_obj(False, lpips_lambda) if cfg.lpips_size else 1
            if cfg.sim_columns >= 2:
                n_obj = prompt_n_obj(cfg.sim_columns, False, bool(cfg.lpips_size) and float(lpips_lambda) == 0.0)
        cfg.n_blocks = len(channels)
        for i, c in enumerate(channels):  # LOW -> HIGH resolution
            cfg.channels[i] = int(c)
        cfg.latent_size, cfg.mapping_layers, cfg.batch_size = latent_size, mapping_layers, batch_size
        cfg.mbstd_group, cfg.use_discriminator, cfg.n_obj = mbstd_group, int(bool(use_discriminator)), n_obj
        cfg.max_pop, cfg.chunk = max_pop, chunk
        if clip_resnet is not None:
            layers, width, res, embed = clip_resnet
            if len(layers) != 4:
                raise ValueError("clip_resnet: layers must hold four stage depths, got %r" % (tuple(layers),))
            cfg.clip_arch = 1
            for i, n in enumerate(layers):
                cfg.clip_rn_layers[i] = int(n)
            clip = (int(width), sum(int(n) for n in layers), int(width) * 32 // 64, 32, int(res), int(embed))
        (cfg.clip_width, cfg.clip_layers, cfg.clip_heads, cfg.clip_patch, cfg.clip_res, cfg.clip_embed) = clip
        cfg.noise_mode, cfg.noise_seed = noise_mode, noise_seed
        cfg.clip_resize, cfg.clip_normalize = int(clip_resize), int(clip_normalize)
        self.cfg = cfg
        self.channels = list(channels)
        self.res = 4 << (len(channels) - 1) if channels else 0
        if biggan is not None:
            self.res = 4 << sum(1 for l in biggan["layers"] if l[0])
        self.n_noise = 1 + 2 * (len(channels) - 1) if channels else 0
        self._h = C.c_void_p()
        _check(self.lib, self.lib.glass_engine_create(C.byref(cfg), C.byref(self._h)))
        self.clip_views = int(clip_views)
        self.latent_space = latent_space
        try:
            if self.clip_views:
                self._call("set_clip_views", self.clip_views, clip_view_permille(clip_view_min), int(bool(clip_view_flip)), int(bool(clip_view_fixed)))
            if latent_space != "z":
                self._call("set_latent_space", latent_space_id(latent_space))
            if latent_space == "sub" and subspace_shape is None:
                raise ValueError('latent_space "sub" needs subspace_shape=(groups, components)')
            if subspace_shape is not None:
                if latent_space != "sub":
                    raise ValueError('subspace_shape belongs to latent_space "sub", not %r' % (latent_space,))
                self.set_subspace_shape(*subspace_shape)
            if float(truncation_psi) != 1.0 or truncation_cutoff is not None:
                self.set_truncation(truncation_psi, truncation_cutoff)
        except Exception:
            self.close()
            raise

    def _call(self, name, *args):
        """glass_engine_<name>(handle, *args); a non-zero status raises RuntimeError with glass_last_error()."""
        _check(self.lib, getattr(self.lib, "glass_engine_" + name)(self._h, *args))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.glass_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- weights -------------------------------------------------------------
    def load_tensor(self, name, array):
        a = _f32(array)
        dims = (C.c_int64 * max(a.ndim, 1))(*a.shape)
        self._call("load_tensor", name.encode(), _fp(a), a.ndim, dims)

    def load_state(self, state):
        for k, v in state.items():
            self.load_tensor(k, np.asarray(v))

    def finalize(self):
        self._call("finalize")

    def set_target(self, feat):
        f = _f32(feat).reshape(-1)
        self._call("set_target", _fp(f), f.size)
        self.n_prompts = 0

    # --- prompt sets -----------------------------------------------------------
    def set_targets(self, features, weights, mode="sum"):
        """A prompt set as the target (include/glass.h "Prompt sets"): features float32 [T, clip_embed], weights [T] (negative: away from the
        entry), mode "sum" (one blended similarity column) or "pareto" (one column per entry; Engine(sim_columns=T)).  After finalize()."""
        f, w = _f32(features), _f32(weights).reshape(-1)
        if f.ndim != 2 or f.shape[0] != w.size:
            raise ValueError("set_targets: features must be [T, clip_embed] with one weight per row, got %r and %d weights" % (f.shape, w.size))
        self._call("set_targets", _fp(f), _fp(w), f.shape[0], f.shape[1], prompt_mode_id(mode))
        self.n_prompts = int(f.shape[0])

    def set_details(self, P):
        """Per-entry similarities [P, T] of the last evaluate() with a prompt set (the means over the views where they are on)."""
        T = int(getattr(self, "n_prompts", 0))
        out = np.empty((P, max(T, 1)), dtype=np.float32)
        self._call("last_set_details", P, _fp(out))
        return out

    def encode_generated(self, images):
        """The CLIP feature a generated image with these pixels gets in the pass: images float32 [n, 3, R, R] in [-1, 1] through the engine's
        own clip_resize / clip_normalize (whole image, no crop views) and the tower -> [n, clip_embed].  n <= max_pop."""
        a = _f32(images)
        if a.ndim != 4 or a.shape[1:] != (3, self.res, self.res):
            raise ValueError("encode_generated: images must be [n, 3, %d, %d], got %r" % (self.res, self.res, a.shape))
        out = np.empty((a.shape[0], self.cfg.clip_embed), dtype=np.float32)
        self._call("encode_generated", _fp(a), a.shape[0], _fp(out))
        return out

    @staticmethod
    def prompt_set_supported(n_entries, mode="sum", sim_columns=0):
        return prompt_set_supported(n_entries, mode, sim_columns)

    # --- image editing (include/glass.h "Image editing") --------------------------
    def set_anchor(self, row):
        """The latent anchor: one row of the current latent space, float32 [floats_per_row].  After finalize(), on Engine(anchor=True)."""
        r = self._rows(np.asarray(row, dtype=np.float32).reshape(1, -1))
        self._call("set_anchor", _fp(r))

    def last_anchor(self, P):
        """The anchor distances [P] of the last evaluate()."""
        d = np.empty((P,), dtype=np.float32)
        self._call("last_anchor", P, _fp(d))
        return d

    def set_direction_source(self, image):
        """The source image of the directional similarity: float32 [3, R, R] in [-1, 1] (the generator's raw range), or None: off.  While
        one is set, the entries of set_targets() are directions.  After finalize()."""
        if image is None:
            self._call("set_direction_source", None)
            return
        a = _f32(image)
        if a.shape != (3, self.res, self.res):
            raise ValueError("set_direction_source: the image must be [3, %d, %d], got %r" % (self.res, self.res, a.shape))
        self._call("set_direction_source", _fp(a))

    def last_direction_source(self):
        """The unit rows [max(clip_views, 1), clip_embed] the last pass subtracted from the candidates' unit features."""
        out = np.empty((max(self.clip_views, 1), self.cfg.clip_embed), dtype=np.float32)
        self._call("last_direction_source", _fp(out))
        return out

    # --- perceptual objective --------------------------------------------------
    def set_lpips_target(self, image):
        """The target of the perceptual objective: float32 [3, S, S] in [-1, 1], S = lpips_size.  After finalize()."""
        a = _f32(image)
        S = int(self.cfg.lpips_size)
        if a.shape != (3, S, S):
            raise ValueError("set_lpips_target: the image must be [3, %d, %d], got %r" % (S, S, a.shape))
        self._call("set_lpips_target", _fp(a), S)

    def lpips(self, x0, x1):
        """LPIPS_VGG16.forward(x0, x1) on caller images float32 [n, 3, S, S] in [-1, 1], through the kernels of the pass -> [n]."""
        a, b = _f32(x0), _f32(x1)
        S = int(self.cfg.lpips_size)
        if a.ndim != 4 or a.shape[1:] != (3, S, S) or b.shape != a.shape:
            raise ValueError("lpips: both image stacks must be [n, 3, %d, %d], got %r and %r" % (S, S, a.shape, b.shape))
        out = np.empty((a.shape[0],), dtype=np.float32)
        self._call("lpips", _fp(a), _fp(b), a.shape[0], _fp(out))
        return out

    def last_lpips(self, P):
        """The distances [P] of the last evaluate()."""
        d = np.empty((P,), dtype=np.float32)
        self._call("last_lpips", P, _fp(d))
        return d

    def encode_text(self, tokens):
        """CLIP.encode_text (clip/model.py:307-320): tokens int [n, ctx] -> float32 [n, clip_embed]."""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.empty((t.shape[0], self.cfg.clip_embed), dtype=np.float32)
        self._call("encode_text", t.ctypes.data_as(ip), t.shape[0], t.shape[1], _fp(out))
        return out

    def encode_image(self, images):
        """CLIP.encode_image on preprocessed images [n,3,R,R] float32 -> [n, clip_embed] (generator.py:26-27)."""
        a = _f32(images)
        out = np.empty((a.shape[0], self.cfg.clip_embed), dtype=np.float32)
        self._call("encode_image", _fp(a), a.shape[0], _fp(out))
        return out

    def gpt2_decode(self, context, length):
        """gpt2/sample.py:21-36 with sample=False: int tokens [P, n] -> [P, n + length] (greedy, fp32)."""
        c = np.ascontiguousarray(context, dtype=np.int32)
        out = np.empty((c.shape[0], c.shape[1] + length), dtype=np.int32)
        self._call("gpt2_decode", c.ctypes.data_as(ip), c.shape[0], c.shape[1], length, out.ctypes.data_as(ip))
        return out

    def gpt2_sample(self, context, length, temperature=0.7, top_k=40, seed=0, generation=0, first_row=0, purpose=0):
        """gpt2/sample.py:21-36 with sample=True: int tokens [P, n] -> [P, n + length], top-k temperature sampling on the device.
        Draws are a function of (seed, generation, purpose, first_row + row, step) and the row's logits (include/glass.h); purpose
        separates the fitness evaluation (GPT2_SAMPLE_EVALUATE) from the save callback (GPT2_SAMPLE_SAVE) of one generation."""
        c = np.ascontiguousarray(context, dtype=np.int32)
        out = np.empty((c.shape[0], c.shape[1] + length), dtype=np.int32)
        self._call("gpt2_sample", c.ctypes.data_as(ip), c.shape[0], c.shape[1], length, float(temperature), int(top_k),
                   int(seed) & 0xFFFFFFFFFFFFFFFF, int(generation), int(first_row), int(purpose), out.ctypes.data_as(ip))
        return out

    # --- device search (include/glass.h "Device search") ------------------------
    def set_search(self, algorithm, pop, xl, xu, eta_c=3.0, eta_m=3.0, prob_m=0.5, seed=1):
        """Between construction and finalize(): turn the device search on for `pop` rows under "ga" / "nsga2" / "cmaes" (sep-CMA-ES: one
        objective; eta_c, eta_m and prob_m are ignored) with scalar bounds xl / xu."""
        if algorithm not in SEARCH_ALGORITHMS:
            raise ValueError("unknown search algorithm %r: expected one of %s" % (algorithm, ", ".join(SEARCH_ALGORITHMS)))
        self._call("set_search", SEARCH_ALGORITHMS[algorithm], int(pop), float(xl), float(xu), float(eta_c), float(eta_m), float(prob_m),
                   int(seed) & 0xFFFFFFFFFFFFFFFF)
        self.search_pop = int(pop)
        self.search_algorithm = algorithm

    def set_search_operators(self, xl, xu, eta_c=3.0, eta_m=3.0, prob_m=0.5, seed=1):
        """Any time after set_search: the values that size nothing (the bounds of a w / w+ search are known only after finalize())."""
        self._call("set_search_operators", float(xl), float(xu), float(eta_c), float(eta_m), float(prob_m), int(seed) & 0xFFFFFFFFFFFFFFFF)

    def set_search_mixed(self, algorithm, pop, n_real, xl, xu, eta_c=3.0, eta_m=3.0, prob_m=0.5, prob_x=0.2, prob_flip=0.01, seed=1):
        """Between construction and finalize(), BigGAN engines: turn the device search on for `pop` mixed rows — n_real (= z_dim) real
        columns with scalar bounds xl / xu, then the class bits, varied by HUX (prob_x per mating) and bit-flip (prob_flip per bit)."""
        if algorithm not in SEARCH_ALGORITHMS:
            raise ValueError("unknown search algorithm %r: expected one of %s" % (algorithm, ", ".join(SEARCH_ALGORITHMS)))
        self._call("set_search_mixed", SEARCH_ALGORITHMS[algorithm], int(pop), int(n_real), float(xl), float(xu), float(eta_c), float(eta_m),
                   float(prob_m), float(prob_x), float(prob_flip), int(seed) & 0xFFFFFFFFFFFFFFFF)
        self.search_pop = int(pop)
        self.search_n_real = int(n_real)

    def set_search_operators_mixed(self, xl, xu, eta_c=3.0, eta_m=3.0, prob_m=0.5, prob_x=0.2, prob_flip=0.01, seed=1):
        """Any time after set_search_mixed: the values that size nothing."""
        self._call("set_search_operators_mixed", float(xl), float(xu), float(eta_c), float(eta_m), float(prob_m), float(prob_x), float(prob_flip),
                   int(seed) & 0xFFFFFFFFFFFFFFFF)

    def set_search_islands(self, islands, migrate_every=0, migrants=1):
        """After set_search / set_search_mixed and before finalize() (include/glass.h "Device search: islands"): `islands` populations of pop
        rows each, island i under seed + i, in one pass per generation; the `migrants` best rows of island i - 1 replace the worst of island i
        every `migrate_every` generations (0: never).  Every search_* buffer then holds islands * pop rows, island-major."""
        self._call("set_search_islands", int(islands), int(migrate_every), int(migrants))
        self.search_islands = int(islands)

    def set_island_weights(self, weights):
        """Own prompts: weights float32 [islands, T] over the T entries of the prompt set (set_targets, mode "sum"; after finalize()).  The
        rows of island i are scored with row i of the table; a single 1 searches that entry alone.  Not with migration, "pareto" or a
        direction source."""
        w = _f32(weights)
        if w.ndim != 2:
            raise ValueError("set_island_weights: weights must be [islands, T], got shape %r" % (w.shape,))
        self._call("set_island_weights", _fp(w), w.shape[0], w.shape[1])

    def search_rows(self):
        """Rows of the device search's buffers: pop, or islands * pop."""
        return self.search_pop * getattr(self, "search_islands", 1)

    def search_init(self, X0):
        """Upload the initial population [pop, floats_per_row] (islands: [islands * pop, floats_per_row], island-major), score it as generation 0
        and rank it."""
        z = self._rows(X0)
        pop = self.search_rows() if hasattr(self, "search_pop") else None      # (None: set_search was never called — the library says so)
        if pop is not None and z.shape[0] != pop:
            raise ValueError("search_init: the initial population must have exactly pop = %d rows, got %d" % (pop, z.shape[0]))
        self._call("search_init", _fp(z))

    def search_init_cma(self, mean, diag=None, sigma=1.0):
        """A "cmaes" search: the distribution of generation 0 — mean [floats_per_row], diag (None: ones) and the step sigma, float64."""
        nv = self.latent_row()[0]
        m = np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)
        d = None if diag is None else np.ascontiguousarray(diag, dtype=np.float64).reshape(-1)
        if m.size != nv or (d is not None and d.size != nv):
            raise ValueError("search_init_cma: mean and diag must hold %d values (a row of latent space %r)" % (nv, self.latent_space))
        self._call("search_init_cma", m.ctypes.data_as(dp), None if d is None else d.ctypes.data_as(dp), float(sigma))

    def search_read_cma(self):
        """The state of a "cmaes" search: dict(mean, diag, p_sigma, p_c float64 [floats_per_row]; sigma, ps_norm; h, finite, updated, skipped,
        updates; best_X float32 [floats_per_row], best_F)."""
        nv = self.latent_row()[0]
        out = {k: np.empty((nv,), np.float64) for k in ("mean", "diag", "p_sigma", "p_c")}
        sd, si = np.empty((2,), np.float64), np.empty((5,), np.int32)
        best_X, best_F = np.empty((nv,), np.float32), np.empty((1,), np.float32)
        self._call("search_read_cma", *[out[k].ctypes.data_as(dp) for k in ("mean", "diag", "p_sigma", "p_c")], sd.ctypes.data_as(dp),
                   si.ctypes.data_as(ip), _fp(best_X), _fp(best_F))
        out.update(sigma=float(sd[0]), ps_norm=float(sd[1]), best_X=best_X, best_F=float(best_F[0]))
        out.update(zip(("h", "finite", "updated", "skipped", "updates"), (int(v) for v in si)))
        return out

    def search_vary(self, generation):
        self._call("search_vary", int(generation))

    def search_evaluate(self, generation, first_row=0, rows=None):
        rows = self.search_rows() - int(first_row) if rows is None else int(rows)
        self._call("search_evaluate", int(generation), int(first_row), rows)

    def search_survive(self, generation):
        self._call("search_survive", int(generation))

    def search_migrate(self, generation):
        """The migration behind search_survive(generation), as a phase of its own (search_step runs it itself); nothing where none is due."""
        self._call("search_migrate", int(generation))

    def search_read_islands(self):
        """int32 [islands, 3]: per island the flagged and the non-finite rows of its last survival and the migrants it accepted last."""
        out = np.empty((getattr(self, "search_islands", 1), 3), np.int32)
        self._call("search_read_islands", out.ctypes.data_as(C.POINTER(C.c_int32)))
        return out

    def search_step(self, generation):
        """One generation on the device: variation, the scoring pass, survival (islands: then the migration, where due); one wait at the end."""
        self._call("search_step", int(generation))

    def search_read(self, *fields, islands=False):
        """dict of the named device-search buffers: "X", "F", "rank", "cd" (the population), "off_X", "off_F", "flags" (the last offspring),
        "counts" = (flagged, non-finite rows of the last survival).  Only what is named is copied back.  An island search returns islands * pop
        rows, island-major; islands=True views every row buffer as [islands, pop, ...]."""
        pop, nv, no = self.search_rows(), self.latent_row()[0], int(self.cfg.n_obj)
        shapes = dict(X=((pop, nv), np.float32), F=((pop, no), np.float32), rank=((pop,), np.int32), cd=((pop,), np.float64),
                      off_X=((pop, nv), np.float32), off_F=((pop, no), np.float32), flags=((pop,), np.int32), counts=((2,), np.int32))
        unknown = [f for f in fields if f not in shapes]
        if unknown:
            raise ValueError("search_read: unknown field(s) %r (expected some of %s)" % (unknown, ", ".join(shapes)))
        out = {f: np.empty(*shapes[f]) for f in fields}
        ctype = {np.float32: C.c_float, np.int32: C.c_int32, np.float64: C.c_double}
        args = [out[f].ctypes.data_as(C.POINTER(ctype[shapes[f][1]])) if f in out else None for f in shapes]
        self._call("search_read", *args)
        if islands:
            K = getattr(self, "search_islands", 1)
            out = {f: a if f == "counts" else a.reshape((K, self.search_pop) + a.shape[1:]) for f, a in out.items()}
        return out

    def latent_uploads(self):
        """(calls, rows): host-to-device latent copies the pass has made on this engine so far."""
        calls, rows = C.c_int64(), C.c_int64()
        self._call("latent_uploads", C.byref(calls), C.byref(rows))
        return calls.value, rows.value

    # --- latent spaces / truncation -------------------------------------------
    def set_latent_space(self, name):
        """Between construction and finalize(): "z", "w", "w+" or "sub" (include/glass.h; "sub" needs set_subspace_shape after it)."""
        self._call("set_latent_space", latent_space_id(name))
        self.latent_space = name

    def set_subspace_shape(self, groups, components):
        """Between set_latent_space("sub") and finalize(): a row is groups * components coefficients."""
        self._call("set_subspace_shape", int(groups), int(components))
        self.subspace_shape = (int(groups), int(components))

    def set_subspace(self, layer_group, basis, base):
        """After finalize(), any time: layer_group int [n_lat] (group of each style layer, -1 = frozen), basis float32 [K, L], base [n_lat, L] or
        [L] (tiled over the layers): dlatents[p][l] = base[l] + c[p][layer_group[l]] . basis (include/glass.h)."""
        G, K = getattr(self, "subspace_shape", (0, 0))
        n_lat, L = self.latent_row()[1], int(self.cfg.latent_size)
        lg = np.ascontiguousarray(layer_group, dtype=np.int32).reshape(-1)
        B, b = _f32(basis), _f32(base)
        if b.shape == (L,):
            b = np.ascontiguousarray(np.broadcast_to(b, (n_lat, L)))
        if lg.shape != (n_lat,) or B.shape != (K, L) or b.shape != (n_lat, L):
            raise ValueError("set_subspace: layer_group [%d], basis [%d, %d] and base [%d, %d] (or [%d]) expected, got %r, %r, %r"
                             % (n_lat, K, L, n_lat, L, L, lg.shape, B.shape, b.shape))
        self._call("set_subspace", lg.ctypes.data_as(C.POINTER(C.c_int32)), _fp(B), _fp(b))

    def expand_latents(self, rows):
        """The dlatents the pass makes its styles from, after truncation: rows [P, floats_per_row] of the engine's space -> float32
        [P, n_lat, L], P <= max_pop (StyleGAN2 engines; the kernels of the pass).  Flattened, a result is a w+ row."""
        z = self._rows(rows)
        n_lat, L = self.latent_row()[1], int(self.cfg.latent_size)
        out = np.empty((z.shape[0], n_lat, L), dtype=np.float32)
        self._call("expand_latents", _fp(z), z.shape[0], _fp(out))
        return out

    @staticmethod
    def subspace_supported(n_lat, latent_size, groups, components, layer_group=None):
        return subspace_supported(n_lat, latent_size, groups, components, layer_group)

    def set_truncation(self, psi, cutoff=None):
        """The truncation trick: dlatents = lerp(dlatent_avg, dlatents, layer_psi); psi in [0, 1], cutoff None = every layer."""
        self._call("set_truncation", float(psi), truncation_cutoff_arg(cutoff))

    def latent_row(self):
        """(floats_per_row, n_lat): what evaluate / generate read per row, and the number of style layers (0: not a StyleGAN2 engine)."""
        if not hasattr(self.lib, "glass_engine_latent_row"):     # (an older A/B build loaded through GLASS_LIB: z rows only)
            return int(self.cfg.latent_size), 0
        w, n = C.c_int32(), C.c_int32()
        self._call("latent_row", C.byref(w), C.byref(n))
        return w.value, n.value

    def map_latents(self, z):
        """Pixel norm + mapping network, untruncated: z float32 [P, latent_size] -> w [P, latent_size], P <= max_pop."""
        z = _f32(z)
        if z.ndim != 2 or z.shape[1] != self.cfg.latent_size:
            raise ValueError("map_latents: z must be [P, %d], got %r" % (self.cfg.latent_size, z.shape))
        out = np.empty_like(z)
        self._call("map_latents", _fp(z), z.shape[0], _fp(out))
        return out

    def _rows(self, x):
        """The population as contiguous float32 rows of the engine's width — checked HERE: the library sees a pointer, and a short row
        would be read past its end."""
        z = _f32(x)
        width = self.latent_row()[0]
        if z.ndim != 2 or z.shape[1] != width:
            raise ValueError("latent rows of space %r must be [P, %d], got %r" % (self.latent_space, width, z.shape))
        return z

    # --- the pass ------------------------------------------------------------
    def _noise_arg(self, noise):
        """noise: list (per minibatch) of lists (per layer) of [res,res] float32 planes."""
        if noise is None:
            return None, None
        flat = [_f32(p) for mb in noise for p in mb]
        arr = (C.POINTER(C.c_float) * len(flat))(*[_fp(p) for p in flat])
        gn = GlassNoise(len(noise), len(noise[0]), arr)
        return gn, (flat, arr)

    def evaluate(self, x, generation=0, first_minibatch=0, noise=None):
        """problem.py:14-29 — returns F float32 [P, n_obj]."""
        z = self._rows(x)
        P = z.shape[0]
        out = np.empty((P, self.cfg.n_obj), dtype=np.float32)
        gn, keep = self._noise_arg(noise)
        self._call("evaluate", _fp(z), P, generation, first_minibatch, C.byref(gn) if gn is not None else None, _fp(out))
        del keep
        return out

    def generate(self, x, generation=0, first_minibatch=0, noise=None):
        """generator.py:29-34 — images float32 [P,3,R,R] in [0,1]."""
        z = self._rows(x)
        P = z.shape[0]
        out = np.empty((P, 3, self.res, self.res), dtype=np.float32)
        gn, keep = self._noise_arg(noise)
        self._call("generate", _fp(z), P, generation, first_minibatch, C.byref(gn) if gn is not None else None, _fp(out))
        del keep
        return out

    def details(self, P):
        feat = np.empty((P, self.cfg.clip_embed), dtype=np.float32)
        dis = np.empty((P,), dtype=np.float32)
        sim = np.empty((P,), dtype=np.float32)
        self._call("last_details", P, _fp(feat), _fp(dis), _fp(sim))
        return dict(features=feat, dis=dis, sim=sim)

    def view_details(self, P):
        """Crop views: per-view outputs of the last evaluate() — features [P, V, embed], sims [P, V], boxes int32 [V, 4] = (x0, y0, s, flip)."""
        V = self.clip_views
        if V < 1:
            raise RuntimeError("crop views are off (Engine(clip_views=...))")
        feat = np.empty((P, V, self.cfg.clip_embed), dtype=np.float32)
        sims = np.empty((P, V), dtype=np.float32)
        boxes = np.empty((V, 4), dtype=np.int32)
        self._call("last_view_details", P, _fp(feat), _fp(sims), boxes.ctypes.data_as(C.POINTER(C.c_int32)))
        return dict(features=feat, sims=sims, boxes=boxes)

    def last_F_device(self, P):
        """The last evaluate()'s fitness rows as a torch CUDA tensor VIEW [P, n_obj] of the engine's own buffer (no copy; valid until the
        engine's next call) — what the RCCL all-gather of a generation sends (parallel.py)."""
        import torch
        ptr = C.c_void_p()
        self._call("last_F_device", P, C.byref(ptr))

        class _View:      # CUDA array interface (v2): torch.as_tensor wraps device memory it does not own
            __cuda_array_interface__ = dict(shape=(P, int(self.cfg.n_obj)), typestr="<f4", data=(int(ptr.value), False), version=2)
        return torch.as_tensor(_View(), device=torch.device("cuda", int(self.cfg.device)))

    def last_gpu_ms(self):
        ms = C.c_float()
        self._call("last_gpu_ms", C.byref(ms))
        return ms.value

    def set_profiling(self, on):
        self._call("set_profiling", int(on))

    def biggan_tap(self, block):
        """Record the activation after GenBlock `block` (-1: after self-attention) on the next pass; see biggan_tap_result."""
        self._call("set_biggan_tap", int(block))

    def biggan_tap_result(self):
        dims = (C.c_int32 * 4)()
        self._call("get_biggan_tap", None, 0, dims)
        out = np.empty(tuple(int(d) for d in dims), dtype=np.float32)
        self._call("get_biggan_tap", _fp(out), out.size, dims)
        return out

    def set_overlap(self, on):
        self._call("set_overlap", int(on))

    def set_profile_filter(self, kernel_substr):
        self._call("set_profile_filter", (kernel_substr or "").encode())

    def profile(self):
        n = C.c_int32()
        self._call("get_profile", None, 0, C.byref(n))
        rows = (ProfRow * max(n.value, 1))()
        self._call("get_profile", rows, n.value, C.byref(n))
        return [dict(name=r.name.decode(), launches=r.launches, total_ms=r.total_ms, flops=r.flops, bytes=r.bytes)
                for r in rows[:n.value]]
