"""The ray service on device memory (prgpu_trace_closest_device / prgpu_trace_any_device / prgpu_ray_service_reserve and
RenderContext.traceRaysDevice / traceShadowRaysDevice), the part that needs no device: the tensor checks of the Python wrapper, the layouts of
the two new structs, and the argument errors every entry point reports before it touches a device.  tests/test_gpu_ray_service_device.py
holds the rest."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from pearray_amd import _cabi as abi
from pearray_amd import backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def rays(n=5):
    return dict(org=torch.zeros((n, 3)), direction=torch.ones((n, 3)), tmin=torch.zeros(n), tmax=torch.ones(n))


def refused(match, **changed):
    kw = dict(rays(), **changed)
    with pytest.raises(ValueError, match=match):
        backend.check_ray_tensors(kw["org"], kw["direction"], kw["tmin"], kw["tmax"], 0)


def test_a_cpu_tensor_is_refused_by_name_and_only_for_being_on_the_cpu():
    """Without a device no tensor can pass; a batch that is right in every other respect is refused for where it lives, and for nothing else --
    which shows that the type, shape, length and contiguity checks before it accept what they should (floats for tmin / tmax included)."""
    refused(r"^org: the tensor is on cpu, not on the GPU")
    refused(r"^org: the tensor is on cpu", tmin=0.0, tmax=float("inf"))
    refused(r"^org: the tensor is on cpu", tmin=1e-4, tmax=5)
    refused(r"^org: the tensor is on cpu", org=torch.zeros((0, 3)), direction=torch.zeros((0, 3)), tmin=torch.zeros(0), tmax=torch.zeros(0))


@pytest.mark.parametrize("name", ["org", "direction", "tmin", "tmax"])
def test_every_argument_is_checked_and_named(name):
    good = rays()[name]
    refused("^%s: float32 is expected, not torch.float64" % name, **{name: good.double()})
    refused("^%s: float32 is expected" % name, **{name: good.to(torch.int32)})
    refused("^%s: a torch tensor is expected, not ndarray" % name, **{name: good.numpy()})
    if good.dim() == 2:
        refused(r"^%s: shape \(n, 3\) is expected, not \(5, 4\)" % name, **{name: torch.zeros((5, 4))})
        refused(r"^%s: shape \(n, 3\) is expected, not \(15,\)" % name, **{name: torch.zeros(15)})
        refused("^%s: the tensor is not contiguous" % name, **{name: torch.zeros((3, 5)).t()})   # a transposed view: shape (5, 3)
    else:
        refused(r"^%s: shape \(n,\) is expected, not \(5, 1\)" % name, **{name: torch.zeros((5, 1))})
        refused("^%s: the tensor is not contiguous" % name, **{name: torch.zeros(10)[::2]})
        refused("^%s: a torch tensor is expected, not bool" % name, **{name: True})
    if name != "org":   # org sets the length
        refused("^%s: 5 rays are expected as in org, not 4" % name, **{name: good[:4].contiguous()})


def test_the_shadow_ray_check_names_the_distance():
    with pytest.raises(ValueError, match="^distance: float32 is expected"):
        r = rays()
        backend.check_ray_tensors(r["org"], r["direction"], r["tmin"], r["tmax"].double(), 0, last="distance")


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of prgpu_rays and prgpu_hits as gcc lays them out equal the ctypes mirror (as tests/test_abi.py does it for the others)."""
    structs = {"prgpu_rays": abi.Rays, "prgpu_hits": abi.Hits}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "prgpu.h"', "int main(void){"]
    for cname, cls in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append("return 0;}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(cls, f).offset, (cname, f)
    assert [f for f, _ in abi.Hits._fields_] == ["entity", "prim", "u", "v", "t", "position", "normal", "tangent", "bitangent", "uv", "material",
                                                "emission", "invalid"]   # the order RenderContext.traceRaysDevice fills them in


def test_null_arguments_are_einval_with_a_message_before_any_device_is_touched():
    lib = abi.load()
    r, h, occ = abi.Rays(), abi.Hits(), (C.c_uint8 * 4)()
    assert lib.prgpu_trace_closest_device(None, None, C.byref(h)) == EINVAL and b"prgpu_trace_closest_device: rays is NULL" in lib.prgpu_last_error()
    assert lib.prgpu_trace_closest_device(None, C.byref(r), None) == EINVAL and b"prgpu_trace_closest_device: hits is NULL" in lib.prgpu_last_error()
    assert lib.prgpu_trace_closest_device(None, C.byref(r), C.byref(h)) == EINVAL and b"prgpu_trace_closest_device: null scene" in lib.prgpu_last_error()
    assert lib.prgpu_trace_any_device(None, None, occ, None) == EINVAL and b"prgpu_trace_any_device: rays is NULL" in lib.prgpu_last_error()
    assert lib.prgpu_trace_any_device(None, C.byref(r), None, None) == EINVAL and b"prgpu_trace_any_device: occluded is NULL" in lib.prgpu_last_error()
    assert lib.prgpu_trace_any_device(None, C.byref(r), occ, None) == EINVAL and b"prgpu_trace_any_device: null scene" in lib.prgpu_last_error()
    assert lib.prgpu_ray_service_reserve(None, 1000) == EINVAL and b"prgpu_ray_service_reserve: null scene" in lib.prgpu_last_error()


def test_the_new_timing_family_is_in_the_header_list():
    header = open(os.path.join(ROOT, "include", "prgpu.h")).read()
    assert '"ao", "vf", "geometry")' in header
