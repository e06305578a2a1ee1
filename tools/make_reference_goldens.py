#!/usr/bin/env python3
"""What the loader makes of the reference's example scenes, for the tests that check it without the reference checkout:

  python tools/make_reference_goldens.py <reference>/examples

writes tests/golden/reference_examples.json (per examples/*.prc the loader's return code and message; the channels of complex.prc's
(output ...) blocks; counts and digests of complex.prc's arrays; the example fixtures' arrays as digests of a fresh conversion; the UV
light spectrum of cornellbox_fluorescent.prc as loaded) and tests/golden/scenes/evaluation.npz (examples/evaluation/scene.prc with its OBJ
meshes, as the loader reads it).  Values only: no scene file is stored."""
import ctypes as C
import glob
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pearray_amd import scene, _cabi as abi  # noqa: E402
import make_example_fixtures as mk  # noqa: E402


def load_results(src_dir):
    """prgpu_prc_load_file on every examples/*.prc, any sky light given a flat table (the Hosek-Wilkie evaluation is the host's)."""
    lib = abi.load()
    table = np.full((256, 512, 11), 0.1, dtype=np.float32)
    sky = (abi.PrcSky * 1)(abi.PrcSky(None, table.ctypes.data_as(C.POINTER(C.c_float)), 512, 256))
    out = {}
    for name in sorted(os.listdir(src_dir)):
        if not name.endswith(".prc"):
            continue
        h = C.c_void_p()
        opt = abi.PrcOptions(0, 0, 0, 1, 0)
        opt.n_skies, opt.skies = 1, sky
        rc = lib.prgpu_prc_load_file(os.path.join(src_dir, name).encode(), C.byref(opt), C.byref(h))
        out[name] = {"rc": rc, "error": "" if rc == 0 else lib.prgpu_prc_last_error().decode()}
        if rc == 0:
            lib.prgpu_prc_free(h)
    return out


def fixture_digests(src_dir):
    """sha256 of every array of a fresh conversion (tools/make_example_fixtures.py) of each example the fixture tool accepts."""
    out = {}
    for f in sorted(glob.glob(os.path.join(src_dir, "*.prc"))):
        name = os.path.basename(f)
        if name in mk.SKIP:
            continue
        try:
            s = mk.load(f)
        except abi.PrgpuError:
            continue
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "x.npz")
            scene.save_scene_npz(p, s.desc, sky_params=s.sky_params())
            z = np.load(p)
            out[name[:-4]] = {k: hashlib.sha256(np.ascontiguousarray(z[k]).tobytes()).hexdigest() for k in sorted(z.files)}
    return out


def main():
    src_dir = sys.argv[1]
    golden = {"generator": "tools/make_reference_goldens.py over the reference's examples/", "load": load_results(src_dir),
              "fixture_digests": fixture_digests(src_dir)}
    s = scene.PrcScene(path=os.path.join(src_dir, "complex.prc"), skies={"sky": np.full((256, 512, 11), 0.5, dtype=np.float32)})
    ch, n = s.outputs()
    golden["complex_outputs"] = [[int(ch[i].kind), ch[i].name.decode()] for i in range(n)]
    shipped = scene.PrcScene(path=os.path.join(src_dir, "complex.prc"))   # as shipped: the loader evaluates the sky model itself
    d = shipped.desc
    sky = [d.lights[i] for i in range(d.n_lights) if d.lights[i].kind == abi.LIGHT_SKY][0]
    tables = np.ctypeslib.as_array(d.spectral_tables, shape=(d.n_spectral_table_values,))
    sha = lambda b: hashlib.sha256(b).hexdigest()   # noqa: E731
    golden["complex"] = dict({f: getattr(d, f) for f in ("n_vertices", "n_triangles", "n_entities", "n_materials", "n_spectra", "n_lights")},
                             sky_table=sha(tables[sky.table_offset:sky.table_offset + 256 * 512 * 11].astype(np.float32).tobytes()),
                             positions=sha(np.ctypeslib.as_array(d.positions, shape=(3 * d.n_vertices,)).astype(np.float32).tobytes()),
                             indices=sha(np.ctypeslib.as_array(d.indices, shape=(3 * d.n_triangles,)).astype(np.uint32).tobytes()),
                             materials=[sha(C.string_at(C.addressof(d.materials[i]), C.sizeof(abi.Material))) for i in range(d.n_materials)])
    src = "(scene (camera :name 'c' :type 'standard') (emission :name 'e' :type 'standard' :radiance (spd 'UVLight.csv')) (material :name 'm' :type 'diffuse'))"
    s = scene.PrcScene(source=src, include_dir=src_dir)
    sp = s.desc.spectra[s.desc.emissions[0].radiance]
    golden["uv_light"] = {"wl_start": sp.wl_start, "wl_end": sp.wl_end,
                          "values": [float(s.desc.spectral_tables[sp.table_offset + i]) for i in range(sp.table_count)]}
    ev = scene.PrcScene(path=os.path.join(src_dir, "evaluation", "scene.prc"))
    golden["evaluation_outputs"] = ev.outputs()[1]
    scene.save_scene_npz(os.path.join(ROOT, "tests", "golden", "scenes", "evaluation.npz"), ev.desc, sky_params=ev.sky_params())
    with open(os.path.join(ROOT, "tests", "golden", "reference_examples.json"), "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
