"""The ray service on the device (RenderContext.traceRays / traceShadowRays = prgpu_trace_closest / prgpu_trace_any) held to the exact
ray / triangle reference: the inputs of tests/test_exact_rays.py (1 - 7, and input 8, the path kernel's primary-hit plane, under R4 and R5)
under rules R1 - R6 of tests/exact_rays.py, with the split traversal and the classic kernel, on four- and on six-wide trees.
tests/test_gpu_bvh_width.py runs inputs 2 and 3 under every top and parity of the tree as well.  The exact classification of an input is computed
once per session (test_exact_rays.case), not once per parametrisation.

Measured on an MI355X host: the whole `-m gpu` suite 583 s (546 tests); before input 8 was added, this module and tests/test_gpu_bvh_width.py together 404 s (164 tests), of which eleven runs of the adversarial-ray body
(one per tree, 33 s each, nearly all of it the checker's side) are 365 s; the slowest case here is 5.8 s (`soup`, which pays for the classification), every
other one under 2 s."""
import numpy as np
import pytest

import test_exact_rays as E
from pearray_amd import backend

pytestmark = pytest.mark.gpu


def run_on_device(name, label=""):
    c = E.case(name)
    g = backend.RenderContext(c.build_scene())
    try:
        info = g.pipelineInfo()
        return E.hold_to_the_rules(c, g.traceRays, g.traceShadowRays, "device %s width %d top %d" % (label, info["bvh_width"], info["bvh_top"]))
    finally:
        g.close()


@pytest.mark.parametrize("width", ["4", "6"])
@pytest.mark.parametrize("split", ["1", "0"])
@pytest.mark.parametrize("name", E.CASES)
def test_the_ray_service_is_held_to_the_exact_reference(monkeypatch, name, split, width):
    monkeypatch.setenv("PRGPU_TRACE_SPLIT", split)
    monkeypatch.setenv("PRGPU_BVH_WIDTH", width)
    run_on_device(name, "split=%s" % split)


def render_on_device(name, label=""):
    c = E.case(name)
    g = backend.RenderContext(c.build_scene())
    try:
        g.render(1)
        g.waitForFinish()
        return E.hold_primary_hits_to_the_rules(c, *g.primaryHits(), label="device " + label)
    finally:
        g.close()


@pytest.mark.parametrize("width", ["4", "6"])
@pytest.mark.parametrize("mode", ["persistent", "lockstep", "streaming"])
@pytest.mark.parametrize("name", E.CAMERA_CASES)
def test_the_path_kernels_primary_hits_are_held_to_the_exact_reference(monkeypatch, name, mode, width):
    monkeypatch.setenv("PRGPU_MODE", mode)
    monkeypatch.setenv("PRGPU_BVH_WIDTH", width)
    render_on_device(name, "mode=%s width=%s" % (mode, width))


def test_the_device_and_the_checker_still_agree_bit_for_bit_on_these_inputs():
    """The rules leave room (margins); the port does not: on the adversarial inputs the device's answers are the checker's."""
    import oracle_binding as ob
    for name in ("aimed", "icosphere-far", "cube-unit", "axes", "windings"):
        c = E.case(name)
        sc = c.build_scene()
        g, o = backend.RenderContext(sc), ob.OracleScene(sc)
        for x, y in zip(g.traceRays(c.org, c.direction, c.tmin, c.tmax), o.trace_closest(c.org, c.direction, c.tmin, c.tmax)):
            assert np.array_equal(x, y), name
        assert np.array_equal(g.traceShadowRays(c.org, c.direction, c.tmin, c.distance), o.trace_any(c.org, c.direction, c.tmin, c.distance)), name
        g.close(); o.close()
