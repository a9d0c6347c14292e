"""Writes tests/golden/lpips_modules.npz: what the reference's own LPIPS_VGG16.forward and Projector._scale_for_lpips compute on seeded
images with the synthetic weights of clip_glass_amd.synth.lpips_state — the pins of tests/lpips_ref.py.  Runs on the CPU, where the
reference is present.  Seeds, small inputs and outputs only: the weights are regenerated from the seed.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_lpips_golden.py

LPIPS_VGG16.__init__ downloads torchvision's VGG16 and the linear weights, and torchvision is absent here (ref_harness stubs it).  The
instance is therefore built without __init__: __new__, nn.Module.__init__, five nn.Sequential slices assembled by hand in VGG16's layer
order (restated: the public configuration D, torchvision's `features` indices), the five bias-free Linear layers and the two buffers —
then the reference's own forward runs.  `layout_source` in the fixture says so.
"""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import ref_harness as rh  # noqa: E402
import lpips_ref as R  # noqa: E402
from clip_glass_amd import synth  # noqa: E402


def load_reference_lpips():
    """(lpips module, Projector class) imported from where the reference lies."""
    rh.load_reference()
    tv = sys.modules["torchvision"]
    if not hasattr(tv, "models"):
        tv.models = types.SimpleNamespace()
    if not hasattr(tv, "datasets"):
        tv.datasets = types.SimpleNamespace(ImageFolder=object)
    ext = types.ModuleType("stylegan2.external_models")
    ext.__path__ = [os.path.join(rh.REF, "stylegan2", "external_models")]
    sys.modules["stylegan2.external_models"] = ext
    ext.lpips = rh._load("stylegan2.external_models.lpips", os.path.join(rh.REF, "stylegan2", "external_models", "lpips.py"),
                         "stylegan2.external_models")
    project = rh._load("stylegan2.project", os.path.join(rh.REF, "stylegan2", "project.py"), "stylegan2")
    return ext.lpips, project.Projector


def build_reference_model(lp, sd):
    m = lp.LPIPS_VGG16.__new__(lp.LPIPS_VGG16)
    nn.Module.__init__(m)
    feats = {}
    for idx, cin, cout in synth.VGG16_CONVS:
        conv = nn.Conv2d(cin, cout, 3, padding=1)
        conv.weight.data.copy_(torch.tensor(sd["lpips.features.%d.weight" % idx]))
        conv.bias.data.copy_(torch.tensor(sd["lpips.features.%d.bias" % idx]))
        feats[idx] = conv
        feats[idx + 1] = nn.ReLU(inplace=False)
    for idx in R.POOL_BEFORE:
        feats[idx - 1] = nn.MaxPool2d(2, 2)
    fi = lp.LPIPS_VGG16._FEATURE_IDX
    m.slices = nn.ModuleList(nn.Sequential(*[feats[j] for j in range(fi[i - 1], fi[i])]) for i in range(1, len(fi)))
    m.linear_layers = nn.ModuleList()
    for k, c in enumerate(synth.LPIPS_SLICE_CHANNELS):
        lin = nn.Linear(c, 1, bias=False)
        lin.weight.data.copy_(torch.tensor(sd["lpips.lin.%d.weight" % k]).view(1, -1))
        m.linear_layers.append(lin)
    m.register_buffer("shift", torch.Tensor([-.030, -.088, -.188]).view(1, -1, 1, 1))
    m.register_buffer("scale", torch.Tensor([.458, .448, .450]).view(1, -1, 1, 1))
    m.pixel_min, m.pixel_max = -1, 1
    m.requires_grad_(False)
    return m.eval()


def reference_outputs():
    assert rh.available(), "needs the reference"
    lp, Projector = load_reference_lpips()
    seed = R.FIXTURE_SEED
    sd = synth.lpips_state(seed)
    m = build_reference_model(lp, sd)
    x32, t32 = R.images(seed, 3, 32, "x32"), R.images(seed, 3, 32, "t32")
    x64 = R.images(seed, 3, 64, "x64")
    proj = types.SimpleNamespace(lpips_size=32)
    out = dict(seed=np.array(seed), x32=x32.astype(np.float16), t32=t32.astype(np.float16), x64=x64.astype(np.float16),
               layout_source=np.array("VGG16 layer order restated by hand (torchvision absent); forward and _scale_for_lpips are the reference's"))
    x32, t32, x64 = (out[k].astype(np.float32) for k in ("x32", "t32", "x64"))      # (stored as fp16: the inputs ARE those values)
    with torch.no_grad():
        out["d_32"] = m(torch.tensor(x32), torch.tensor(t32)).numpy()
        out["d_32_shared"] = m(torch.tensor(x32), torch.tensor(t32[:1]).expand(3, -1, -1, -1)).numpy()
        a64 = Projector._scale_for_lpips(proj, torch.tensor(x64))
        out["area_64_0"] = a64[0].numpy()      # (the first image's: enough to pin the box mean)
        out["d_64"] = m(a64, torch.tensor(t32)).numpy()
    return out


def main():
    out = reference_outputs()
    np.savez_compressed(R.FIXTURE, **out)
    print({k: np.asarray(v).shape for k, v in out.items()}, out["d_32"], out["d_64"], os.path.getsize(R.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
