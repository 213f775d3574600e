#!/usr/bin/env python3
"""Loads the reference's text_lowres.obj (data/obj/text/text_lowres.obj of the reference tree, with its text.mtl) through
the OBJ path of obj.load_obj_scene and stores the flattened triangle arrays and material rows in
tests/golden/text_lowres_obj.npz.  tests/test_host_logic.py checks the packed mesh the package ships
(data/text_lowres.npz) against them, so that test needs no file outside the repository.

    python tests/golden/make_obj_fixture.py <reference tree>/data/obj/text/text_lowres.obj
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from hslu_i.ba_raytracing.f2501_raytracer_amd.obj import load_obj_scene  # noqa: E402

KEYS = ("tri_v1", "tri_e1", "tri_e2", "tri_normal", "materials")

if __name__ == "__main__":
    if len(sys.argv) != 2 or not sys.argv[1].endswith(".obj"):
        raise SystemExit(__doc__)
    f = load_obj_scene(sys.argv[1], None).flatten()
    np.savez_compressed(os.path.join(HERE, "text_lowres_obj.npz"), **{k: getattr(f, k) for k in KEYS})
    print({k: getattr(f, k).shape for k in KEYS})
