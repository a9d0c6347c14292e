"""Writes tests/golden/dlatent_modules.npz: what the reference's own Generator computes on the `mini` network (32 px, L = 32, n_lat = 8)
under the truncation trick and for explicit dlatents — the pins of tests/dlatent_ref.py and of the engine's w / w+ / psi modes.  Runs on
the CPU, where the reference is present.  Outputs and small inputs only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_dlatent_golden.py

lerp: ref_harness stubs stylegan2.utils with a placeholder lerp (truncation was off everywhere until now).  This script loads the
reference's real stylegan2/utils.py beside the stub (yaml and PIL resolve here; torchvision is the harness's stub, given the one more
attribute the module touches at import) and hands ITS lerp to the stub module that models.py calls; where that import fails, the fallback is the function's fp32 behaviour restated: the 0 / 1
shortcuts, then torch.lerp.  `lerp_source` in the fixture says which one produced it.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import ref_harness as rh  # noqa: E402
import dlatent_ref as R  # noqa: E402


def install_reference_lerp():
    """Replace the harness's placeholder; returns "reference" or "restated"."""
    rh.load_reference()
    stub = sys.modules["stylegan2.utils"]
    try:
        import types
        tv = sys.modules["torchvision"]            # (the harness's stub; utils.py subclasses torchvision.datasets.ImageFolder at import)
        if not hasattr(tv, "datasets"):
            tv.datasets = types.SimpleNamespace(ImageFolder=object)
        real = rh._load("stylegan2._utils_real", os.path.join(rh.REF, "stylegan2", "utils.py"), "stylegan2")
        stub.lerp = real.lerp
        return "reference"
    except Exception:
        import numbers

        def lerp(a, b, beta):
            if isinstance(beta, numbers.Number):
                if beta == 1:
                    return b
                if beta == 0:
                    return a
            return torch.lerp(a, b, beta)
        stub.lerp = lerp
        return "restated"


def reference_outputs():
    """dict name -> ndarray: the reference Generator's outputs on R.fixture_inputs()."""
    assert rh.available(), "needs the reference"
    source = install_reference_lerp()
    sd, z, avg, planes = R.fixture_inputs()
    G = rh.build_ref_G(sd, R.MINI["channels"], R.MINI["latent"], R.MINI["mapping"])
    zt = torch.tensor(z)
    out = dict(z=z, dlatent_avg=avg, lerp_source=np.array(source))
    for i, p in enumerate(planes):
        out["noise_%d" % i] = np.asarray(p, np.float32)
    with torch.no_grad():
        G.dlatent_avg.copy_(torch.tensor(avg))
        G(zt)                                                  # noise layers learn their shapes
        G.static_noise(noise_tensors=[torch.tensor(p)[None, None] for p in planes])
        w = G.G_mapping(zt)
        out["w"] = w.numpy()
        for name, (psi, cutoff) in R.MODES.items():
            G.set_truncation(truncation_psi=psi, truncation_cutoff=cutoff)
            out["img_z_" + name] = G(latents=zt).numpy()
        G.set_truncation(truncation_psi=None)
        out["img_w"] = G(dlatents=w).numpy()
        w_plus = R.fixture_w_plus(w.numpy())
        out["w_plus"] = w_plus
        out["img_w_plus"] = G(dlatents=torch.tensor(w_plus)).numpy()
        G.set_truncation(truncation_psi=0.5, truncation_cutoff=3)
        out["img_w_plus_psi05_cut3"] = G(dlatents=G.truncate(torch.tensor(w_plus))).numpy()
    return out


def main():
    out = reference_outputs()
    np.savez_compressed(R.FIXTURE, **out)
    print({k: np.asarray(v).shape for k, v in out.items()}, "lerp:", out["lerp_source"], os.path.getsize(R.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
