"""The host half of the batched renderer (include/rsx.h: rsx_render_*): frame size and the static field image against
rsoccer_amd/Render/raster.py, the views, and the refusals.  No device needed."""
import ctypes as C

import numpy as np
import pytest

from rsoccer_amd import _lib as L
from rsoccer_amd.Render import SSL_VIEW, VSS_VIEW, FieldRaster, view_for_field

# field tables of the engine (get_field_params() of VSS 3v3 / 5v5 and SSL division A), as far as a view needs them
VSS_3V3 = dict(length=1.5, width=1.3, penalty_length=0.15, penalty_width=0.7, goal_width=0.4, goal_depth=0.1, ball_radius=0.0215, rbt_radius=0.0375)
VSS_5V5 = dict(length=2.2, width=1.8, penalty_length=0.15, penalty_width=0.8, goal_width=0.4, goal_depth=0.15, ball_radius=0.0215, rbt_radius=0.0375)
SSL_DIV_A = dict(length=12.0, width=9.0, penalty_length=1.8, penalty_width=3.6, goal_width=1.8, goal_depth=0.18, ball_radius=0.0215, rbt_radius=0.09)


def _views():
    out = []
    for base, scales in ((VSS_VIEW, (500, 100, 64, 37.5)), (SSL_VIEW, (100, 20, 12.5))):
        for s in scales:
            out.append(dict(base, scale=s))
    out.append(view_for_field(L.KIND_VSS, VSS_5V5, scale=40))
    out.append(view_for_field(L.KIND_SSL, SSL_DIV_A, scale=40))
    return out


VIEWS = _views()
IDS = [f"{'vss' if v['square'] else 'ssl'}-{v['length']}m-{v['scale']}" for v in VIEWS]


@pytest.mark.parametrize("view", VIEWS, ids=IDS)
def test_frame_size_is_the_rasterisers(view):
    w, h = FieldRaster(view).window_size
    assert L.render_size(view) == (h, w)


@pytest.mark.parametrize("view", VIEWS, ids=IDS)
def test_field_image_equals_the_rasterisers_byte_for_byte(view):
    """both sides evaluate the same double-precision expressions (same libm hypot): equality, not a tolerance"""
    want = FieldRaster(view)._field
    got = L.render_field(view)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), int((got != want).any(axis=2).sum())


def test_views():
    assert view_for_field(L.KIND_VSS, VSS_3V3) == VSS_VIEW
    assert view_for_field(L.KIND_VSS, VSS_3V3, scale=64) == dict(VSS_VIEW, scale=64)
    assert L.render_view_reference(L.KIND_VSS) == VSS_VIEW and L.render_view_reference(L.KIND_SSL) == SSL_VIEW
    a = view_for_field(L.KIND_SSL, SSL_DIV_A)
    assert (a["length"], a["width"], a["pen_len"], a["pen_wid"], a["goal_wid"]) == (12.0, 9.0, 1.8, 3.6, 1.8)
    assert (a["margin"], a["circle"], a["scale"], a["square"], a["robot"]) == (0.35, 1.0, 100, False, 0.09)
    from rsoccer_amd.Entities import Field
    full = dict({k: 0.0 for k in L.FIELD_KEYS}, **VSS_5V5)
    assert view_for_field(L.KIND_VSS, Field(**full)) == view_for_field(L.KIND_VSS, VSS_5V5)   # a Field works like the dict


@pytest.mark.parametrize("change,word", [
    (dict(length=float("nan")), "finite"), (dict(ball=float("inf")), "finite"),
    (dict(scale=0.0), "scale"), (dict(scale=-5.0), "scale"),
    (dict(scale=5000.0), "4096"), (dict(scale=2.0), "8 and"), (dict(length=1e300), "4096"),
])
def test_invalid_views_are_refused_with_a_message(change, word):
    lib = L.load()
    v = L.RenderView.from_dict(dict(VSS_VIEW, **change))
    w, h = C.c_int(-1), C.c_int(-1)
    assert lib.rsx_render_size(C.byref(v), C.byref(w), C.byref(h)) == -1       # RSX_ERR_ARG
    assert word in lib.rsx_last_error().decode()
    buf = np.zeros(16, np.uint8)
    assert lib.rsx_render_field(C.byref(v), buf.ctypes.data_as(C.c_void_p)) == -1
    assert not buf.any()
    with pytest.raises(L.RsxError, match=word):
        L.render_size(dict(VSS_VIEW, **change))
    with pytest.raises(ValueError):
        L.RenderView.from_dict({k: v for k, v in VSS_VIEW.items() if k != "ball"})


def test_no_frames_without_a_device():
    """rsx_render_open / rsx_render are device calls like every other: no handle, no frames (there is no CPU fallback)"""
    lib = L.load()
    v = L.RenderView.from_dict(VSS_VIEW)
    assert lib.rsx_render_open(None, C.byref(v), None) == -1 and "null handle" in lib.rsx_last_error().decode()
    buf = np.zeros(64, np.uint8)
    assert lib.rsx_render(None, None, 1, 0, buf.ctypes.data_as(C.c_void_p), None) == -1
    n = C.c_int64(7)
    assert lib.rsx_render_errors(None, C.byref(n), None) == -1 and n.value == 7
    assert not buf.any()
    if L.device_count() == 0:
        with pytest.raises(L.RsxError):
            L.Sim(L.KIND_VSS, 0, 3, 3, 25, 4, 0)
        from rsoccer_amd.vec import VecVSSEnv
        with pytest.raises(L.RsxError):
            VecVSSEnv(4).render()
