#!/usr/bin/env python3
"""Regenerate the v4 fixtures in tests/golden/ (v4_ref_*.npz) from the reference's OWN v4 code.

Needs the reference next to the repository (oracle/build_ref.sh's REF) and a CPU with AVX2 and FMA; the
reference never travels, these fixtures (data: inputs + recorded outputs) do.  Steps:
  1. oracle/build_ref.sh compiles demofox_path_tracing_optimization_v4.cpp :1-1556 inside
     oracle/ref_v4.cpp, once per flag variant of global_preprocessor_flags.h (oracle/_ref/ref_v4_*).
  2. Every case of tests/v4_ref.CASES is one fresh process of its variant's binary: 64 x 48 in
     16 x 16 tiles, the calls of DemofoxRenderOptV4 it names on a zeroed accumulator.
  3. A case's file holds the tiled accumulator exactly as RenderTile wrote it (acc), the final iFrame,
     OutputToScreen's pixels where the case has them (screen), and the inputs that are the case's own
     (scene arrays, camera as px, py, pz, distance).  The two env maps are stored once, in
     v4_ref_env_equirect.npz / v4_ref_env_cubemap.npz.  Each file stays under 256 KB.
  4. manifest.json "v4_ref": the flag diffs and hashes oracle/build_ref.sh recorded, and each case's
     parameters and SHA-256 of its accumulator bytes.
"""
from __future__ import annotations

import hashlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

MAX_BYTES = 256 * 1024


def main() -> None:
    subprocess.run([str(ROOT / "oracle" / "build_ref.sh")], check=True)
    import v4_ref as vr
    if not vr.ref_available():
        sys.exit("make_golden_v4.py: oracle/_ref/ref_v4_* were not built (reference absent, or no AVX2/FMA)")
    envs = {k: vr.synth_env(k) for k in ("equirect", "cubemap")}
    for k, e in envs.items():
        np.savez_compressed(HERE / f"v4_ref_env_{k}.npz", env=e)
    scene = (vr.SCENE_QUADS, vr.SCENE_SPHERES, vr.SCENE_MATS)
    cases = {}
    for name, c in vr.CASES.items():
        kind = vr.VARIANTS[c["variant"]][0]
        cam = vr.camera_args(c["cam"]) if c["cam"] else None
        r = vr.run_ref(c["variant"], frames=c["frames"], frame0=c["frame0"], env=envs.get(kind),
                       scene=scene if c["edited"] else None, cam=cam, screen=c["screen"])
        arrays = {"acc": r["acc"], "iframe": r["iframe"]}
        if c["screen"]:
            arrays["screen"] = r["screen"]
        if c["edited"]:
            arrays.update(quads=scene[0], spheres=scene[1], mats=scene[2])
        if cam is not None:
            arrays["cam"] = np.array(cam, np.float32)
        np.savez_compressed(vr.fixture_path(name), **arrays)
        cases[name] = {**c, "env": kind, "width": vr.W, "height": vr.H, "tile": [vr.TW, vr.TH],
                       "iframe": float(r["iframe"][0]), "sha256_acc": hashlib.sha256(r["acc"].tobytes()).hexdigest()}
    for p in sorted(HERE.glob("v4_ref_*.npz")):
        assert p.stat().st_size <= MAX_BYTES, f"{p.name} is {p.stat().st_size} bytes"
    mpath = HERE / "manifest.json"
    manifest = json.loads(mpath.read_text())
    manifest["v4_ref"] = {
        "generator": "tests/golden/make_golden_v4.py (oracle/_ref/ref_v4_* = the reference's v4 lines 1-1556)",
        "layout": "acc: the reference's tiled planar-8 accumulator, flat f32; screen: H x W u32 0x00RRGGBB",
        "flags": json.loads((ROOT / "oracle" / "_ref" / "v4_flags.json").read_text()),
        "cases": cases,
    }
    mpath.write_text(json.dumps(manifest, indent=1) + "\n")
    print(json.dumps(manifest["v4_ref"]["cases"], indent=1))


if __name__ == "__main__":
    main()
