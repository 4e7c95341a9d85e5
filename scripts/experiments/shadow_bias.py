#!/usr/bin/env python3
"""The default relative bias of sf_trace_shadow_to (sf_shadow_defaults), chosen on the CPU oracle.

For fixtures t1..t4 (the oracle's own frames) and the three lights of the shadow tests, every surface pixel's ray
from the light is traced once with the oracle (tests/shadowcheck.py); the definition's predicate min_t < len (1 - b)
is then evaluated for b = 0 and every power of two from 2^-16 to 2^-4. A pixel is SELF-SHADOWED at b when it is
shadowed and the light-side ray's nearest sphere is the sphere the camera saw there (the same heap index): the only
"occluder" is the pixel's own sphere, met a hair before the pixel because the two traversals round differently. A
pixel FACES THE LIGHT BY MORE THAN 30 DEGREES when the light stands more than 30 degrees above its tangent plane:
n . (l - w) / |l - w| > sin 30 = 0.5. The default is the smallest power of two with no self-shadowed pixel among
those, over all fixtures and lights. (Nearer to grazing the own sphere's far side legitimately comes first, and
the Lambert term is small anyway.)

Run from the repository root after the build: python scripts/experiments/shadow_bias.py [--json out.json]
"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (REPO, os.path.join(REPO, "sphereflake-raytracer_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

from oracle import pyoracle   # noqa: E402
from rayscheck import frame   # noqa: E402
from sphereflake_amd import lights   # noqa: E402
import shadowcheck as sc   # noqa: E402

EXPONENTS = list(range(-16, -3))


def main():
    rows = []
    worst = {e: 0 for e in EXPONENTS}
    for name in ("t1", "t2", "t3", "t4"):
        S = pyoracle.load_setup(name)
        f = frame(name)
        for light_name, light in sc.LIGHTS.items():
            mint, idx = sc.oracle_shadow_rays(S["children"], f["pos4"], S["origin"], light)
            d, length, surf = lights.shadow_model(f["pos4"], S["origin"], light, 0.0)
            n = f["nrm4"][..., :3]
            with np.errstate(invalid="ignore", divide="ignore"):
                lam = -(n * d).sum(-1) / length
            facing = surf & (lam > 0.5)
            own = surf & (idx == f["index"])
            row = {"fixture": name, "light": light_name, "surface": int(surf.sum()), "facing": int(facing.sum()),
                   "self": {}, "shadowed": {}}
            for e in [None] + EXPONENTS:
                b = 0.0 if e is None else 2.0 ** e
                vis = sc.vis_of(f["pos4"], S["origin"], light, b, mint)
                k = int(((vis == 0) & own & facing).sum())
                row["self"]["0" if e is None else f"2^{e}"] = k
                row["shadowed"]["0" if e is None else f"2^{e}"] = int((vis == 0).sum())
                if e is not None:
                    worst[e] += k
            rows.append(row)
            print(name, light_name, "surface", row["surface"], "facing > 30 deg", row["facing"], "self-shadowed:",
                  " ".join(f"{k}:{v}" for k, v in row["self"].items()))
    chosen = min(e for e in EXPONENTS if all(worst[g] == 0 for g in EXPONENTS if g >= e))
    print("self-shadowed facing pixels over all cases:", " ".join(f"2^{e}:{worst[e]}" for e in EXPONENTS))
    print(f"smallest power of two with none (and none above it): 2^{chosen}")
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fp:
            json.dump({"cases": rows, "total_self_shadowed_facing": {f"2^{e}": worst[e] for e in EXPONENTS},
                       "chosen": f"2^{chosen}"}, fp, indent=1)


if __name__ == "__main__":
    main()
