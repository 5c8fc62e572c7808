from rsoccer_amd.Render.raster import SSL_VIEW, VSS_VIEW, FieldRaster  # noqa: F401

_KIND_VSS = 0


def reference_view(kind):
    """the reference's fixed window of a robot class (0 = VSS, 1 = SSL): ``VSS_VIEW`` / ``SSL_VIEW``"""
    return VSS_VIEW if kind == _KIND_VSS else SSL_VIEW


def view_for_field(kind, field, scale=None):
    """A view dict (``raster.py``'s format) that shows the whole of ``field`` — a handle's ``get_field_params()`` dict or an
    ``Entities.Field`` — for the fields the reference's fixed window does not contain (VSS 5v5, SSL division A / hardware challenge).

    Length, width, penalty area, goal and ball radius come from the field, and so does the radius of an SSL robot; margin, centre
    circle, px/m and the robot shape are those of the class's reference view.  A VSS robot is drawn as the 8 cm cube it is: its half
    side is the class's (the field's ``rbt_radius`` is the 3.75 cm wheel-base circle, not the body).  For the VSS 3v3 field the
    result is ``VSS_VIEW`` itself; ``scale`` overrides the px/m."""
    f = field if isinstance(field, dict) else vars(field)
    ref = reference_view(kind)
    view = dict(length=f["length"], width=f["width"], margin=ref["margin"], circle=ref["circle"],
                pen_len=f["penalty_length"], pen_wid=f["penalty_width"], goal_wid=f["goal_width"], goal_dep=f["goal_depth"],
                scale=ref["scale"] if scale is None else scale,
                robot=ref["robot"] if ref["square"] else f["rbt_radius"], ball=f["ball_radius"], square=ref["square"])
    return view
