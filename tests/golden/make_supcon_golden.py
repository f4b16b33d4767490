"""Generate the SupCon / SimCLR fixtures by running the REFERENCE losses.py on the CPU (build
container only; never at test time, never on the GPU box).

    python tests/golden/make_supcon_golden.py REFERENCE_DIR   # writes tests/golden/supcon/supcon_*.npz

(a directory of their own: tests/golden_io.py takes every *.npz directly under tests/golden for a
fixture of the layer.)

The reference's losses.py is imported in place from REFERENCE_DIR (or $GLL_REFERENCE_DIR).
Each fixture holds fp32 unit-norm features [bsz, V, d], labels (absent: SimCLR), the settings,
the reference's float64 loss and autograd gradient on those fp32 values, and the reference's OWN
float32 loss and gradient errors against that float64 run (recorded, not asserted: the yardstick
of what fp32 arithmetic of this loss costs).
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

# name, bsz, V, d, classes (0: SimCLR), mode, T, Tb
CASES = [
    ("all_lab_v2", 150, 2, 64, 10, "all", 0.07, 0.07),
    ("one_lab_v2", 150, 2, 64, 10, "one", 0.07, 0.07),
    ("all_simclr_v2_t05", 120, 2, 48, 0, "all", 0.5, 0.07),
    ("one_simclr_v3", 40, 3, 16, 0, "one", 0.07, 0.07),
    ("all_lab_v3_t05", 50, 3, 33, 5, "all", 0.5, 0.07),
    ("all_lab_v1", 96, 1, 33, 6, "all", 0.07, 0.07),
    ("one_lab_v1", 96, 1, 20, 6, "one", 0.07, 0.07),
    ("c0_v1", 8, 1, 5, -1, "all", 0.07, 0.07),      # one singleton label: c_r = 0, NaN
]


def load_reference(ref_dir):
    spec = importlib.util.spec_from_file_location("reference_losses", os.path.join(ref_dir, "losses.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(mod, f, y, mode, T, Tb, dtype):
    x = torch.from_numpy(f).to(dtype).requires_grad_(True)
    crit = mod.SupConLoss(temperature=T, contrast_mode=mode, base_temperature=Tb)
    loss = crit(x, None if y is None else torch.from_numpy(y))
    loss.backward()
    return loss.detach().double().item(), x.grad.double().numpy()


def main():
    ref_dir = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GLL_REFERENCE_DIR")
    if not ref_dir:
        sys.exit("make_supcon_golden: give the reference checkout's directory")
    mod = load_reference(ref_dir)
    for n, (name, bsz, V, d, classes, mode, T, Tb) in enumerate(CASES):
        rng = np.random.default_rng(1700 + n)
        f = rng.standard_normal((bsz, V, d))
        if classes > 0:   # class structure, so that the positives matter
            y = (np.arange(bsz) % classes).astype(np.int64)
            rng.shuffle(y)
            f += 1.5 * rng.standard_normal((classes, 1, d))[y]
        elif classes < 0:
            y = np.array([0, 0, 1, 1, 1, 2, 0, 1], dtype=np.int64)[:bsz]   # label 2 is alone
        else:
            y = None
        f = (f / np.linalg.norm(f, axis=-1, keepdims=True)).astype(np.float32)
        l64, g64 = run(mod, f, y, mode, T, Tb, torch.float64)
        l32, g32 = run(mod, f, y, mode, T, Tb, torch.float32)
        with np.errstate(invalid="ignore"):
            e_loss = abs(l32 - l64)
            e_grad = float(np.linalg.norm(g32 - g64) / np.linalg.norm(g64))
        out = dict(features=f, mode=mode, T=np.float64(T), Tb=np.float64(Tb), loss64=np.float64(l64),
                   grad64=g64, ref32_loss_err=np.float64(e_loss), ref32_grad_relerr=np.float64(e_grad))
        if y is not None:
            out["labels"] = y
        os.makedirs(os.path.join(HERE, "supcon"), exist_ok=True)
        np.savez_compressed(os.path.join(HERE, "supcon", f"supcon_{name}.npz"), **out)
        print(f"supcon_{name}: loss {l64:.12g}  fp32 loss err {e_loss:.2e}  fp32 grad rel err {e_grad:.2e}")


if __name__ == "__main__":
    main()
