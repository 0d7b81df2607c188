"""The architect, orthographic and angular cameras (src/cameras/ of the
reference) next to the perspective one.

CPU: yk_scene_set_camera's constructor / setAxis arithmetic against a numpy
float32 / float64 restatement in source order, bit for bit; the appended ABI
fields; the refusals.
GPU: the device ray generators through yk_debug_camera_rays against the same
kind of restatement; an upright architect camera against the perspective
oracle; orthographic frames against traced restated rays; the angular
camera's samples without a ray (wt = 0); batch, pipe, shard, merge and handle
invariance; the perspective path against the oracle.

None of the three cameras is pinned against reference output (no fixture
uses them): the restatements here are the source's operation order.
Frames are 48 x 32 (non-square: resx and resy cannot be swapped unnoticed),
tile_size 16.
"""
import ctypes as C

import numpy as np
import pytest

from core_amd import _abi as A
from core_amd.scene import Scene, probe_scene
from oracle import oracle as O
from oracle.oracle import Oracle
from tests.dl_common import fcos, fsin
from tests.scenes import specular
from tests.test_photon_gpu import pm_params

F, D = np.float32, np.float64
W, H, TILE = 48, 32, 16
PERSP, ARCH, ORTHO, ANG = (A.YK_CAMERA_PERSPECTIVE, A.YK_CAMERA_ARCHITECT, A.YK_CAMERA_ORTHOGRAPHIC,
                           A.YK_CAMERA_ANGULAR)
DEG = 0.01745329251994329576922
# a frame looking up the Cornell box's y axis whose camera_t::camY is (0, 0, -1)
# in every bit (test_upright_frame_has_exact_camy), so that architectCam_t's
# vup = aspect_ratio * (0, 0, -1) is perspectiveCam_t's aspect_ratio * camY
UPRIGHT = dict(from_=(0.0625, 0.125, -0.25), to=(0.0625, 1.125, -0.25), up=(0.0625, 0.125, 0.75))
FRONT = dict(from_=(0, 1, -3.6), to=(0, 1, 0), up=(0, 2, -3.6))  # the Cornell generator's own view
BG = ((0.2, 0.3, 0.45), 0.8)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(a, b):
    return bool((_bits(a) == _bits(b)).all())


def _state_bytes(st):
    return bytes(st)


# ---------------------------------------------------------------- restatement

def _v(x):
    return np.array(x, F)


def _cross(a, b):
    return _v([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _normalize(a):  # vector3d_t::normalize, vector3d.h:249-260
    ln = a[0] * a[0] + a[1] * a[1] + a[2] * a[2]
    if ln != 0:
        ln = F(1.0) / np.sqrt(ln)
        a = _v([a[0] * ln, a[1] * ln, a[2] * ln])
    return a


def restate_state(type_, from_, to, up, resx=W, resy=H, focal=1.0, aspect_ratio=1.0, near_clip=0.0, far_clip=-1.0,
                  aperture=0.0, dof_distance=0.0, bokeh_type=0, bokeh_bias=0, bokeh_rotation=0.0, scale=1.0,
                  angle=90.0, max_angle=None, circular=True, mirrored=False):
    """camera_t's constructor (camera.h:43-66), then the camera's own
    constructor, setAxis and factory tail, as a dict of yk_camera_state fields"""
    pos, look, upp = _v(from_), _v(to), _v(up)
    aspect = F(aspect_ratio) * F(resy) / F(resx)
    camY, camZ = upp - pos, look - pos
    camX = _cross(camZ, camY)
    camY = _cross(camZ, camX)
    camX, camY, camZ = _normalize(camX), _normalize(camY), _normalize(camZ)
    o = dict(position=pos, cam_z=camZ, near_p=pos + camZ * F(near_clip), far_p=pos + camZ * F(far_clip),
             resx=resx, resy=resy, aperture=F(0), dof_distance=F(0), dof_rt=_v([0, 0, 0]), dof_up=_v([0, 0, 0]),
             bokeh_type=0, bokeh_bias=0, lens_ls=np.zeros(16, F), kind=PERSP, hor_phi=F(0), max_r=F(0),
             circular=0, aspect_ratio=F(0), camY=camY, camX=camX)
    if type_ == ORTHO:  # orthographicCamera.cc:37-49; the factory's double scale through a PFLOAT argument
        sc = F(scale)
        vright, vup = camX, aspect * camY
        o.update(vto=camZ, position=pos - F(0.5 * D(sc)) * (vup + vright), vup=vup * (sc / F(resy)),
                 vright=vright * (sc / F(resx)), kind=ORTHO)
        return o
    if type_ == ANG:  # angularCamera.cc:27-47 and the factory's tail :96-98
        ang = F(angle)
        o.update(hor_phi=F(D(ang) * 3.14159265358979323846 / D(F(180.0))), vright=camX * F(-1.0) if mirrored else camX,
                 vup=camY, vto=camZ, max_r=F(D(angle if max_angle is None else max_angle) / D(angle)),
                 circular=int(bool(circular)), aspect_ratio=aspect, kind=ANG)
        return o
    # perspectiveCam_t ctor + setAxis (perspectiveCamera.cc:29-71); architectCam_t::setAxis
    # (architectCamera.cc:54-68) replaces camY by (0, 0, -1) in vup alone
    ap = F(aperture)
    ls = np.zeros(16, F)
    if 3 <= bokeh_type <= 6:
        w = F(D(F(bokeh_rotation)) * DEG)
        wi = F(6.28318530717958647692 / D(F(bokeh_type)))
        for i in range(0, (bokeh_type + 2) * 2, 2):
            ls[i], ls[i + 1] = fcos(w), fsin(w)
            w = F(w + wi)
    vright = camX
    vup = aspect * (_v([0, 0, -1]) if type_ == ARCH else camY)
    vto = camZ * F(focal) - F(0.5) * (vup + vright)
    o.update(aperture=ap, dof_distance=F(dof_distance), dof_rt=ap * camX, dof_up=ap * camY, bokeh_type=bokeh_type,
             bokeh_bias=bokeh_bias, lens_ls=ls, vto=vto, vup=vup * (F(1.0) / F(resy)),
             vright=vright * (F(1.0) / F(resx)))
    return o


def state_struct(o):
    st = A.yk_camera_state()
    for k in ("position", "vright", "vup", "vto", "cam_z", "near_p", "far_p", "dof_rt", "dof_up"):
        setattr(st, k, A.f3(*[float(x) for x in o[k]]))
    for k in ("resx", "resy", "bokeh_type", "bokeh_bias", "kind", "circular"):
        setattr(st, k, int(o[k]))
    for k in ("aperture", "dof_distance", "hor_phi", "max_r", "aspect_ratio"):
        setattr(st, k, float(o[k]))
    st.lens_ls = (C.c_float * 16)(*[float(x) for x in o["lens_ls"]])
    return st


def _vec(o, k, n, dt=F):
    return np.broadcast_to(np.array(o[k], dt), (n, 3))


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _clip(o, frm, d, dt=F):
    """ray_plane_intersection (geometry.h:33-36) with the near and far planes"""
    n = len(d)
    cz = _vec(o, "cam_z", n, dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        den = _dot(d, cz)
        return _dot(cz, _vec(o, "near_p", n, dt) - frm) / den, _dot(cz, _vec(o, "far_p", n, dt) - frm) / den


def _normalize_cam(d):
    """the camera ray's normalize() as the device states it (yk_math.h: (y*y + z*z) + x*x)"""
    ln = (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) + d[:, 0] * d[:, 0]
    return d * (F(1.0) / np.sqrt(ln))[:, None]


def shoot_perspective(o, px, py, lu, lv):
    """perspectiveCam_t::shootRay (perspectiveCamera.cc:127-149); polygon bokeh, no bias"""
    n = len(px)
    d = (px[:, None] * _vec(o, "vright", n) + py[:, None] * _vec(o, "vup", n)) + _vec(o, "vto", n)
    d = _normalize_cam(d)
    frm = _vec(o, "position", n).copy()
    tmin, tmax = _clip(o, frm, d)
    if o["aperture"] != 0:
        bt, ls = o["bokeh_type"], o["lens_ls"]
        assert 3 <= bt <= 6 and o["bokeh_bias"] == 0
        fn = F(bt)
        idx = (lu * fn).astype(np.int32)
        r1 = (lu - idx.astype(F) / fn) * fn
        r1 = np.sqrt(r1)  # biasDist, BB_NONE
        b1 = r1 * lv
        b0 = r1 - b1
        idx = idx << 1
        u = ls[idx] * b0 + ls[idx + 2] * b1
        v = ls[idx + 1] * b0 + ls[idx + 3] * b1
        LI = u[:, None] * _vec(o, "dof_rt", n) + v[:, None] * _vec(o, "dof_up", n)
        frm = frm + LI
        d = _normalize_cam(o["dof_distance"] * d - LI)
    return frm, d, tmin, tmax, np.ones(n, F)


def shoot_ortho(o, px, py):
    """orthoCam_t::shootRay (orthographicCamera.cc:52-64)"""
    n = len(px)
    frm = (_vec(o, "position", n) + _vec(o, "vright", n) * px[:, None]) + _vec(o, "vup", n) * py[:, None]
    d = _vec(o, "vto", n).copy()
    tmin, tmax = _clip(o, frm, d)
    return frm, d, tmin, tmax, np.ones(n, F)


def _fsin64(x):
    """fSin's formula (mathOptimizations.h:249-268) evaluated in float64"""
    x = np.array(x, D)
    two_pi, pi = 6.28318530717958647692, 3.14159265358979323846
    m = (x > two_pi) | (x < -two_pi)
    x = np.where(m, x - np.trunc(x * 0.15915494309189533577) * two_pi, x)
    x = np.where(x < -pi, x + two_pi, np.where(x > pi, x - two_pi, x))
    x = (1.27323954473516268615 * x) - ((0.40528473456935108578 * x) * np.abs(x))
    return np.clip(x + (np.abs(x) - 1.0) * (0.225 * x), -1.0, 1.0)


def shoot_angular(o, px, py, dt=F):
    """angularCam_t::shootRay (angularCamera.cc:49-71) in float32 (source
    order) or, dt = float64, the same formulas on the same inputs in double.
    -> from, dir, radius, wt; dir is 0 where wt is 0"""
    n = len(px)
    px, py = px.astype(dt), py.astype(dt)
    sin, cos = (fsin, fcos) if dt is F else (_fsin64, lambda x: _fsin64(x + 1.57079632679489661923))
    u = dt(1.0) - dt(2.0) * (px / dt(o["resx"]))
    v = dt(2.0) * (py / dt(o["resy"])) - dt(1.0)
    v = v * dt(o["aspect_ratio"])
    radius = np.sqrt(u * u + v * v)
    dead = (radius > dt(o["max_r"])) if o["circular"] else np.zeros(n, bool)
    theta = np.where((u == 0) & (v == 0), dt(0.0), np.arctan2(v, u)).astype(dt)
    phi = radius * dt(o["hor_phi"])
    d = sin(phi)[:, None] * (cos(theta)[:, None] * _vec(o, "vright", n, dt) + sin(theta)[:, None] * _vec(o, "vup", n, dt)) \
        + cos(phi)[:, None] * _vec(o, "vto", n, dt)
    d = np.where(dead[:, None], dt(0.0), d).astype(dt)
    return _vec(o, "position", n, dt).copy(), d, radius, np.where(dead, F(0.0), F(1.0)).astype(F)


def sample_positions(p, spp, multipass=False, pass_off=0):
    """renderTile's film positions (integrator.cc:262-292) of the render area's
    pixels, row-major, sample fastest -> px, py (float32, (h, w, spp))"""
    L = O.lib()
    d1 = F(1.0 / D(F(spp)))
    px = np.zeros((p.height, p.width, spp), F)
    py = np.zeros_like(px)
    for y in range(p.height):
        for x in range(p.width):
            j, i = p.xstart + x, p.ystart + y
            so = L.orc_fnv((i * L.orc_fnv(j)) & 0xFFFFFFFF)
            for s in range(spp):
                dx = dy = F(0.5)
                if multipass:
                    dx, dy = F(L.orc_ri_vdc(pass_off + s, so)), F(L.orc_ri_s(pass_off + s, so))
                elif spp > 1:
                    dx, dy = (F(0.5) + F(s)) * d1, F(L.orc_ri_lp((s + so) & 0xFFFFFFFF, 0))
                px[y, x, s], py[y, x, s] = F(j) + dx, F(i) + dy
    return px, py


# ---------------------------------------------------------------------- scenes

def cornell(integrator, cam, background=None, builder=None):
    """the Cornell generator's scene (or builder's) with camera `cam`"""
    if builder is None:
        s = Scene()
        p = s.generate(integrator, W, H)
    else:
        s, p = builder(W, H, integrator)
    kw = dict(resx=W, resy=H)
    kw.update(cam)
    s.set_camera(**kw)
    if background is not None:
        s.set_background(*background)
    s.build()
    return s, p


def frame(p, spp=2, crop=None, **kw):
    q = p.copy()
    q.xstart, q.ystart, q.width, q.height = crop or (0, 0, W, H)
    q.tile_size = TILE
    q.aa_samples = spp
    q.filter = A.YK_FILTER_BOX
    q.aa_pixelwidth = 1.0
    for k, v in kw.items():
        setattr(q, k, v)
    return q


ARCH_CAM = dict(type=ARCH, focal=0.7, **UPRIGHT)
ARCH_DOF = dict(type=ARCH, focal=0.7, aperture=0.05, dof_distance=1.8, bokeh_type=A.YK_BOKEH_PENTA, bokeh_rotation=17.0,
                near_clip=0.1, far_clip=10.0, **UPRIGHT)
ORTHO_CAM = dict(type=ORTHO, scale=2.4, near_clip=0.05, far_clip=50.0, **UPRIGHT)
# looking down from between the ceiling and the light quad, whose material emits upwards
ORTHO_DOWN = dict(type=ORTHO, scale=2.4, from_=(0.0625, 1.99, -0.25), to=(0.0625, 0.99, -0.25), up=(0.0625, 1.99, 0.75))
ANG_CAM = dict(type=ANG, angle=90.0, max_angle=45.0, circular=True, **FRONT)
ANG_MIRROR = dict(type=ANG, angle=75.0, max_angle=37.5, circular=True, mirrored=True, near_clip=0.2, far_clip=30.0,
                  aspect_ratio=1.25, **FRONT)
ANG_FULL = dict(type=ANG, angle=180.0, circular=False, **FRONT)


# ------------------------------------------------------------------------- CPU

def test_upright_frame_has_exact_camy():
    o = restate_state(PERSP, **UPRIGHT)
    assert o["camY"].tobytes() == _v([0, 0, -1]).tobytes()  # +0, +0, -1: also the zeros' signs


CASES = {"perspective": dict(type=PERSP, focal=1.3, **FRONT),
         "perspective_dof": dict(type=PERSP, focal=1.3, aperture=0.08, dof_distance=4.2, bokeh_type=A.YK_BOKEH_TRI,
                                 bokeh_bias=A.YK_BOKEH_BIAS_EDGE, bokeh_rotation=-33.0, near_clip=0.5, far_clip=20.0,
                                 aspect_ratio=1.1, **FRONT),
         "architect": dict(type=ARCH, focal=1.1, from_=(0.3, 0.9, -3.2), to=(0.1, 1.0, 0.2), up=(0.3, 1.9, -3.1)),
         "architect_dof": ARCH_DOF, "orthographic": ORTHO_CAM,
         "orthographic_tilted": dict(type=ORTHO, scale=0.37, aspect_ratio=0.9, from_=(0.3, 0.9, -3.2),
                                     to=(0.1, 1.0, 0.2), up=(0.3, 1.9, -3.1), near_clip=1.0, far_clip=7.5),
         "angular": ANG_CAM, "angular_mirrored": ANG_MIRROR, "angular_full": ANG_FULL,
         "angular_odd": dict(type=ANG, angle=33.3, max_angle=71.7, circular=True, **UPRIGHT)}


@pytest.mark.parametrize("name", list(CASES))
def test_parameters_to_state(name):
    """camera_state() is the numpy restatement of the constructor and setAxis,
    bit for bit, and survives yk_scene_set_camera_state"""
    cam = dict(CASES[name])
    s = Scene()
    s.set_camera(resx=W, resy=H, **cam)
    type_ = cam.pop("type")
    want = state_struct(restate_state(type_, **cam))
    got = s.camera_state()
    gb, wb = _state_bytes(got), _state_bytes(want)
    for k, _ in A.yk_camera_state._fields_:  # field by field first, for a readable failure
        f = getattr(A.yk_camera_state, k)
        assert gb[f.offset:f.offset + f.size] == wb[f.offset:f.offset + f.size], (name, k)
    assert gb == wb, name
    if type_ == ANG:
        mr = cam.get("max_angle", cam["angle"]) / cam["angle"]
        assert got.max_r == F(mr) and got.hor_phi == F(D(F(cam["angle"])) * np.pi / 180.0)
        assert got.kind == ANG and got.circular == int(cam["circular"])
    t = Scene()
    t.set_camera_state(got)
    assert _state_bytes(t.camera_state()) == _state_bytes(got)
    assert s.camera().type == type_  # the parameter-level getter keeps the type as given


def test_zero_tail_is_todays_perspective_camera():
    """A yk_camera whose appended part is zero is the perspective camera: the
    state's leading part is what the perspective constructor gives, offsets
    unchanged, and the state's appended part is zero."""
    assert A.yk_camera.type.offset == 80 and A.yk_camera.scale.offset == 96 and C.sizeof(A.yk_camera) == 120
    assert A.yk_camera_state.kind.offset == 196 and C.sizeof(A.yk_camera_state) == 216
    c = A.yk_camera(A.f3(*FRONT["from_"]), A.f3(*FRONT["to"]), A.f3(*FRONT["up"]), W, H, 1.3, 1.0, 0.0, -1.0, 0.08, 4.2,
                    A.YK_BOKEH_HEXA, 0, 12.0)  # the fields earlier callers set; the rest zero
    s = Scene()
    A.check(A.lib().yk_scene_set_camera(s.handle, C.byref(c)))
    got = _state_bytes(s.camera_state())
    want = _state_bytes(state_struct(restate_state(PERSP, focal=1.3, aperture=0.08, dof_distance=4.2,
                                                   bokeh_type=A.YK_BOKEH_HEXA, bokeh_rotation=12.0, **FRONT)))
    assert got == want and got[196:] == bytes(20)
    t, p = probe_scene("cornell_pt", W, H)  # the generator's camera: zero-initialised tail as well
    assert _state_bytes(t.camera_state())[196:] == bytes(20) and t.camera().type == PERSP


def test_upright_architect_state_is_the_perspective_state():
    for extra in ({}, dict(aperture=0.05, dof_distance=1.8, bokeh_type=A.YK_BOKEH_PENTA, bokeh_rotation=17.0)):
        a, b = Scene(), Scene()
        a.set_camera(resx=W, resy=H, focal=0.7, type=ARCH, **UPRIGHT, **extra)
        b.set_camera(resx=W, resy=H, focal=0.7, type=PERSP, **UPRIGHT, **extra)
        assert _state_bytes(a.camera_state()) == _state_bytes(b.camera_state())
    a, b = Scene(), Scene()  # any other frame: architect differs
    a.set_camera(resx=W, resy=H, type=ARCH, **FRONT)
    b.set_camera(resx=W, resy=H, type=PERSP, **FRONT)
    assert _state_bytes(a.camera_state()) != _state_bytes(b.camera_state())


def test_set_camera_refusals():
    s = Scene()

    def code(**kw):
        a = dict(resx=W, resy=H, **FRONT)
        a.update(kw)
        try:
            s.set_camera(**a)
        except A.YkError as e:
            return e.code
        return A.YK_OK

    assert code(type=4) == A.YK_ERR_UNSUPPORTED and code(type=-1) == A.YK_ERR_UNSUPPORTED
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert code(type=ORTHO, scale=bad) == A.YK_ERR_ARG, bad
        assert code(type=ANG, angle=bad) == A.YK_ERR_ARG, bad
    for bad in (-1e-9, float("nan"), float("inf")):
        assert code(type=ANG, max_angle=bad) == A.YK_ERR_ARG, bad
    assert code(type=ANG, max_angle=0.0) == A.YK_OK
    assert code(type=ORTHO, aperture=0.1) == A.YK_ERR_ARG and code(type=ANG, aperture=0.1) == A.YK_ERR_ARG
    assert code(type=ARCH, aperture=0.1) == A.YK_OK and code(type=ORTHO, scale=1e-3) == A.YK_OK
    # the parameters of another kind are not read
    assert code(type=PERSP, scale=-1.0, angle=-1.0, max_angle=-1.0) == A.YK_OK
    assert code(type=ORTHO, angle=-1.0, max_angle=-1.0) == A.YK_OK
    st = s.camera_state()
    for kind, ap, want in ((7, 0.0, A.YK_ERR_UNSUPPORTED), (-1, 0.0, A.YK_ERR_UNSUPPORTED),
                           (ORTHO, 0.1, A.YK_ERR_ARG), (ANG, 0.1, A.YK_ERR_ARG), (ARCH, 0.1, A.YK_OK)):
        st.kind, st.aperture = kind, ap
        assert A.lib().yk_scene_set_camera_state(s.handle, C.byref(st)) == want, (kind, ap)
    assert s.camera_state().kind == PERSP  # an architect camera's shootRay is the perspective one's


# ------------------------------------------------------------------------- GPU

def camera_rays(dev, px, py, lu=None, lv=None):
    """yk_debug_camera_rays (include/yk_test_hooks_camera.h), bound here: the
    hook is not part of the product ABI table. -> (n, 8) rays, wt"""
    f = A.lib().yk_debug_camera_rays
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, A.fp, C.c_int64, C.c_void_p, A.fp]
    n = len(px)
    inp = np.zeros((n, 4), F)
    inp[:, 0], inp[:, 1] = px, py
    inp[:, 2], inp[:, 3] = (0.5 if lu is None else lu), (0.5 if lv is None else lv)
    rays = np.full((n, 8), np.nan, F)
    wt = np.full(n, np.nan, F)
    A.check(f(dev._p, inp.ctypes.data_as(A.fp), n, rays.ctypes.data, wt.ctypes.data_as(A.fp)))
    return rays, wt


def film_positions(o=None, n_rim=6000, seed=5):
    """~20k film positions: the pixel centres, the four corners, the exact
    centre (u = v = 0 for the angular camera), random positions with sub-pixel
    offsets and, for an angular state o, positions on its circle's rim at
    relative distances 1e-7 .. 1e-2 either side of max_r"""
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    px = [jj.ravel() + 0.5, [0, W, 0, W], [W / 2.0]]
    py = [ii.ravel() + 0.5, [0, 0, H, H], [H / 2.0]]
    n_rand = 12000
    px.append(rng.uniform(0, W, n_rand))
    py.append(rng.uniform(0, H, n_rand))
    if o is not None:
        th = rng.uniform(-np.pi, np.pi, n_rim)
        # 60 of the 6000 as close as 1e-7 (where float32 and float64 may disagree), the rest 1e-5 .. 1e-2
        ex = np.where(np.arange(n_rim) < 60, -7.0, rng.uniform(-5, -2, n_rim))
        r = D(o["max_r"]) * (1.0 + rng.choice([-1.0, 1.0], n_rim) * 10.0 ** ex)
        u, v = r * np.cos(th), r * np.sin(th)
        px.append((1.0 - u) * 0.5 * W)
        py.append((v / D(o["aspect_ratio"]) + 1.0) * 0.5 * H)
    return np.concatenate(px).astype(F), np.concatenate(py).astype(F)


def _upload(dev, monkeypatch, cam, integrator="cornell_dl", background=None, builder=None):
    monkeypatch.setenv("YK_DEBUG_HOOKS", "1")
    for k in ("YK_PIPES", "YK_BATCH_SAMPLES", "YK_MERGE", "YK_SPLIT", "YK_SMALL", "YK_BATCH_GB"):
        monkeypatch.delenv(k, raising=False)
    s, p = cornell(integrator, cam, background, builder)
    dev.upload(s)
    return s, p


def _render(dev, q, shard=(0, 1)):
    film = dev.new_film(q)
    st = dev.render_shard(q, film, *shard)
    return film.cpu().numpy(), st


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["architect", "architect_dof", "orthographic", "orthographic_tilted"])
def test_ray_generators_bit_exact(gpu_device, monkeypatch, name):
    cam = dict(CASES[name])
    _upload(gpu_device, monkeypatch, cam)
    type_ = cam.pop("type")
    o = restate_state(type_, **cam)
    px, py = film_positions()
    rng = np.random.default_rng(11)
    lu, lv = rng.random(len(px)).astype(F), rng.random(len(px)).astype(F)
    rays, wt = camera_rays(gpu_device, px, py, lu, lv)
    frm, d, tmin, tmax, wt_r = shoot_ortho(o, px, py) if type_ == ORTHO else shoot_perspective(o, px, py, lu, lv)
    assert len(px) >= 13000
    assert _same(wt, wt_r) and _same(rays[:, 0:3], frm) and _same(rays[:, 3:6], d), name
    assert _same(rays[:, 6], tmin) and _same(rays[:, 7], tmax), name
    if type_ == ORTHO:  # dir = vto = camZ as stored, not normalised again
        assert _same(rays[:, 3:6], np.broadcast_to(o["cam_z"], d.shape))


# Largest |dir component| deviation of the numpy float32 restatement of
# angularCam_t::shootRay from the float64 evaluation of the same formulas on
# the inputs of film_positions(), measured on the CPU (the test measures it
# again and asserts it is within the constant): 5.60e-7, 5.45e-7 and 9.63e-7
# for the three cameras below, rounded up here. The device may deviate four
# times as far: its atan2f differs from numpy's by a few ulp of theta, which
# fSin / fCos pass on.
ANGULAR_F32_DEV = {"angular": 5.7e-7, "angular_mirrored": 5.5e-7, "angular_full": 9.7e-7}
ANGULAR_DIR_BOUND = {k: 4 * v for k, v in ANGULAR_F32_DEV.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["angular", "angular_mirrored", "angular_full"])
def test_angular_ray_generator(gpu_device, monkeypatch, name):
    cam = dict(CASES[name])
    _upload(gpu_device, monkeypatch, cam)
    cam.pop("type")
    o = restate_state(ANG, **cam)
    px, py = film_positions(o)
    assert len(px) >= 19000
    rays, wt = camera_rays(gpu_device, px, py)
    frm, d32, r32, wt32 = shoot_angular(o, px, py, F)
    _, d64, r64, wt64 = shoot_angular(o, px, py, D)
    assert _same(wt, wt32) and _same(rays[:, 0:3], frm), name
    centre = (px == W / 2.0) & (py == H / 2.0)
    # u = v = 0: theta = 0 without atan2, so the float32 restatement holds bit for bit (fCos(0) * vto)
    assert centre.sum() == 1 and _same(rays[centre, 3:6], d32[centre])
    if o["circular"]:
        assert 0.2 < (wt == 0).mean() < 0.8
        dead = wt == 0  # the reference's default ray_t, direction 0
        assert (rays[dead, 3:6] == 0).all() and (rays[dead, 6] == 0).all() and (rays[dead, 7] == -1).all()
    else:
        assert (wt == 1).all()
    agree = wt32 == wt64  # both sides of max_r alike in float32 and float64
    assert (~agree).mean() <= 0.01, (~agree).sum()
    live = agree & (wt32 == 1)
    own = np.abs(d32[live].astype(D) - d64[live]).max()
    got = np.abs(rays[live, 3:6].astype(D) - d64[live]).max()
    print(f"{name}: {len(px)} positions, {(~agree).sum()} left out; float32 restatement within {own:.3e} of "
          f"float64, device within {got:.3e} (bound {ANGULAR_DIR_BOUND[name]:.2e})")
    assert own <= ANGULAR_F32_DEV[name]
    assert got <= ANGULAR_DIR_BOUND[name]
    # tmin / tmax: ray_plane_intersection on the direction the device made
    lv = wt == 1
    tmin, tmax = _clip(o, rays[lv, 0:3], rays[lv, 3:6])
    assert _same(rays[lv, 6], tmin) and _same(rays[lv, 7], tmax)


@pytest.mark.gpu
@pytest.mark.parametrize("integrator", ["cornell_dl", "cornell_pt"])
@pytest.mark.parametrize("dof", [False, True])
def test_upright_architect_equals_perspective_oracle(gpu_device, monkeypatch, integrator, dof):
    cam = dict(ARCH_DOF if dof else ARCH_CAM)
    if dof:
        cam.update(near_clip=0.0, far_clip=-1.0)
    s, p = _upload(gpu_device, monkeypatch, cam, integrator)
    t, _ = cornell(integrator, dict(cam, type=PERSP))
    orc = Oracle(t)
    for crop in (None, (5, 3, 40, 27)):
        q = frame(p, 2, crop)
        film, st = _render(gpu_device, q)
        _, sums, cnt = orc.render(q)
        assert (film.view(np.uint32) == sums.view(np.uint32)).all(), (integrator, dof, crop)
        assert st.closest_rays == cnt["closest"] and st.shadow_rays == cnt["shadow"]
        assert st.camera_samples == q.width * q.height * 2


@pytest.mark.gpu
@pytest.mark.parametrize("integrator", ["cornell_dl", "cornell_pt"])
def test_orthographic_end_to_end(gpu_device, monkeypatch, integrator):
    cam = dict(ORTHO_DOWN)
    s, p = _upload(gpu_device, monkeypatch, cam, integrator)
    cam.pop("type")
    o = restate_state(ORTHO, **cam)
    q = frame(p, 1, transp_background=1)
    px, py = sample_positions(q, 1)
    frm, d, tmin, tmax, _ = shoot_ortho(o, px.ravel(), py.ravel())
    rays = np.concatenate([frm, d, tmin[:, None], tmax[:, None]], 1).astype(F)
    prim = gpu_device.split_hits(gpu_device.trace_closest(gpu_device.rays_to_device(rays)))[0].reshape(H, W)
    film, st = _render(gpu_device, q)
    hit = prim >= 0
    assert 0.3 < hit.mean() < 0.95  # the film overhangs the box: hits and misses
    assert ((film[:, :, 3] == 1) == hit).all() and (film[~hit, 3] == 0).all() and (film[:, :, 4] == 1).all()
    e, ms = s.export(), s.material_states()
    lightp = hit & np.isin(prim, np.flatnonzero([ms[m].type == A.YK_MAT_LIGHT for m in e["tri_material"]]))
    assert lightp.sum() >= 8
    lm = next(m for m in ms if m.type == A.YK_MAT_LIGHT)
    # lightMat_t::emit: lightCol on the side the normal points to (wo * N > 0), nothing else
    # is added on a material without a diffuse component
    facing = _dot(-d.reshape(H, W, 3)[lightp], e["tri_normal"][prim[lightp]]) > 0
    assert facing.all() and not lm.double_sided
    assert _same(film[lightp][:, 0:3], np.broadcast_to(_v(list(lm.color)), (int(lightp.sum()), 3)))
    assert (film[~hit, 0:3] == 0).all()
    assert st.camera_samples == W * H
    if integrator == "cornell_dl":
        assert st.closest_rays == W * H


def _dead_case(name):
    if name == "dl":
        return "cornell_dl", None, lambda p: p
    if name == "pt":
        return "cornell_pt", None, lambda p: p
    if name == "pm":
        return "cornell_pt", None, lambda p: pm_params(p, photons=2000, fg_samples=2)
    if name == "dl_spec":  # the specular recursion's node pipeline
        return "cornell_dl", (lambda w, h, integ: specular(w, h, integ, raydepth=2)), lambda p: p
    raise ValueError(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dl", "pt", "pm", "dl_spec"])
def test_angular_dead_samples(gpu_device, monkeypatch, name):
    """Weights: imageFilm_t::addSample hands a sample that sits on a pixel edge
    to the neighbouring pixel as well (3 of these 1536 pixels at 2 spp, with
    any camera), so "weight = spp" holds for all but those. The weight plane
    is therefore held, for every pixel and bit for bit, against the one the
    same frame gives with circular = 0, where every sample carries a ray: a
    dead sample adds exactly its filter weight."""
    integrator, builder, par = _dead_case(name)
    weights = {}
    s, p = _upload(gpu_device, monkeypatch, dict(ANG_CAM, circular=False), integrator, BG, builder)
    for crop in ((None, (5, 3, 40, 27)) if name == "dl" else (None,)):
        q = frame(par(p), 2, crop, transp_background=0)
        if name == "pm":
            gpu_device.photon_build(q)
        film, st = _render(gpu_device, q)
        assert st.camera_samples == q.width * q.height * 2
        weights[crop] = film[:, :, 4].copy()
        assert (film[:, :, 3] == film[:, :, 4]).all()  # every sample: alpha 1, with its weight
    s, p = _upload(gpu_device, monkeypatch, ANG_CAM, integrator, BG, builder)
    cam = dict(ANG_CAM)
    cam.pop("type")
    o = restate_state(ANG, **cam)
    spp = 2
    crops = (None, (5, 3, 40, 27)) if name == "dl" else (None,)
    for crop in crops:
        base = frame(par(p), spp, crop)
        if name == "pm":
            gpu_device.photon_build(base)
        px, py = sample_positions(base, spp)
        wt = shoot_angular(o, px.ravel(), py.ravel())[3].reshape(px.shape)
        nlive = int((wt == 1).sum())
        dead_px = (wt == 0).all(axis=2)
        assert dead_px.sum() > 100 and (wt == 1).all(axis=2).sum() > 100 and 0 < nlive < wt.size
        stats = []
        for tb in (0, 1):
            q = frame(base, spp, crop, transp_background=tb)
            film, st = _render(gpu_device, q)
            w0 = weights[crop]
            own = w0 == spp  # pixels that hold their own samples and no neighbour's
            assert own.mean() > 0.99 and (dead_px & own).sum() > 100
            assert (film[:, :, 4].view(np.uint32) == w0.view(np.uint32)).all(), (name, tb)
            assert (film[dead_px & own] == np.array([0, 0, 0, 0, spp], F)).all(), (name, tb)
            assert (film[dead_px][:, 0:4] == 0).all(), (name, tb)
            if not tb:  # opaque background: alpha 1 for every sample with a ray, 0 for the others
                assert (film[own, 3] == (wt == 1).sum(axis=2)[own]).all(), name
            assert st.camera_samples == nlive, (st.camera_samples, nlive)
            stats.append(st)
        a, b = stats
        for f in ("closest_rays", "shadow_rays", "closest_nodes", "closest_tris", "shadow_nodes", "shadow_tris"):
            assert getattr(a, f) == getattr(b, f), f
        if name == "dl":
            # the camera rays of the live samples alone: the device's own rays, traced as a query
            lv = wt.ravel() == 1
            rays, wt_d = camera_rays(gpu_device, px.ravel()[lv], py.ravel()[lv])
            assert (wt_d == 1).all()
            qs = A.yk_stats()
            gpu_device.trace_closest(gpu_device.rays_to_device(rays), qs)
            assert (a.closest_rays, a.closest_nodes, a.closest_tris) == (nlive, qs.closest_nodes, qs.closest_tris)


@pytest.mark.gpu
def test_angular_without_circle_has_no_dead_sample(gpu_device, monkeypatch):
    s, p = _upload(gpu_device, monkeypatch, dict(ANG_CAM, circular=False), "cornell_pt", BG)
    for spp in (1, 3):
        film, st = _render(gpu_device, frame(p, spp, transp_background=0))
        assert st.camera_samples == W * H * spp
        # alpha 1 per sample; all but the few pixels that get an edge sample of a neighbour hold spp samples
        assert (film[:, :, 3] == film[:, :, 4]).all() and (film[:, :, 4] >= spp).all()
        assert (film[:, :, 4] == spp).mean() > 0.99


@pytest.mark.gpu
def test_angular_gauss_filter_and_adaptive_passes_repeat(gpu_device, monkeypatch):
    s, p = _upload(gpu_device, monkeypatch, ANG_CAM, "cornell_pt", BG)
    q = frame(p, 2, filter=A.YK_FILTER_GAUSS, aa_pixelwidth=3.0, aa_passes=2, aa_inc_samples=1, aa_threshold=0.05)
    a, sa = _render(gpu_device, q)
    b, sb = _render(gpu_device, q)
    assert (a.view(np.uint32) == b.view(np.uint32)).all()
    assert (sa.camera_samples, sa.closest_rays, sa.shadow_rays) == (sb.camera_samples, sb.closest_rays, sb.shadow_rays)
    px, py = sample_positions(q, 2, multipass=True)
    wt = shoot_angular(restate_state(ANG, **{k: v for k, v in ANG_CAM.items() if k != "type"}), px.ravel(),
                       py.ravel())[3]
    assert sa.camera_samples >= (wt == 1).sum() and np.isfinite(a).all()
    # far outside the circle (beyond the filter's reach) nothing but weight arrives
    assert (a[0, 0, 0:4] == 0).all() and a[0, 0, 4] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["architect_dof", "orthographic", "angular"])
def test_new_cameras_do_not_depend_on_batches_pipes_shards_merge_or_handles(gpu_device, monkeypatch, name):
    from core_amd.device import Device
    s, p = _upload(gpu_device, monkeypatch, CASES[name], "cornell_pt", BG)
    q = frame(p, 2, bounces=3)
    base, st0 = _render(gpu_device, q)
    fields = ("closest_rays", "shadow_rays", "closest_nodes", "closest_tris", "shadow_nodes", "shadow_tris",
              "camera_samples")

    def check(film, st, tag):
        assert (film.view(np.uint32) == base.view(np.uint32)).all(), (name, tag)
        for f in fields:
            assert getattr(st, f) == getattr(st0, f), (name, tag, f)

    monkeypatch.setenv("YK_BATCH_SAMPLES", str(TILE * TILE * 2))  # one tile per batch
    for pipes in ("1", "4"):
        monkeypatch.setenv("YK_PIPES", pipes)
        check(*_render(gpu_device, q), f"one-tile batches, {pipes} pipes")
    monkeypatch.delenv("YK_BATCH_SAMPLES")
    monkeypatch.setenv("YK_PIPES", "1")
    check(*_render(gpu_device, q), "1 pipe")
    monkeypatch.delenv("YK_PIPES")
    monkeypatch.setenv("YK_MERGE", "0")
    check(*_render(gpu_device, q), "unmerged")
    monkeypatch.delenv("YK_MERGE")
    f0, s0 = _render(gpu_device, q, (0, 2))
    f1, s1 = _render(gpu_device, q, (1, 2))
    assert ((f0 + f1).view(np.uint32) == base.view(np.uint32)).all(), name  # box filter: disjoint pixels
    for f in fields:
        assert getattr(s0, f) + getattr(s1, f) == getattr(st0, f), (name, f)
    other = Device(0)
    try:
        other.upload(s)
        film, st = Device.render_multi([gpu_device, other], q)
        check(film, st, "two handles")
    finally:
        other.close()


@pytest.mark.gpu
def test_perspective_path_unchanged_against_oracle(gpu_device, monkeypatch):
    """type = 0: film and every counter of an existing parity form (the
    Cornell path-tracing probe, here with a crop and a thin lens)"""
    for cam in (dict(type=PERSP, focal=1.3, **FRONT), CASES["perspective_dof"]):
        s, p = _upload(gpu_device, monkeypatch, cam, "cornell_pt")
        orc = Oracle(s)
        q = frame(p, 3, (5, 3, 40, 27))
        film, st = _render(gpu_device, q)
        _, sums, cnt = orc.render(q)
        assert (film.view(np.uint32) == sums.view(np.uint32)).all()
        assert (st.closest_rays, st.shadow_rays, st.closest_nodes, st.closest_tris, st.shadow_nodes, st.shadow_tris) == \
            (cnt["closest"], cnt["shadow"], cnt["closest_nodes"], cnt["closest_tris"], cnt["shadow_nodes"],
             cnt["shadow_tris"])
        assert st.camera_samples == 40 * 27 * 3
        if cam.get("aperture", 0) == 0:  # the hook's rays are the oracle's camera rays
            rays, wt = camera_rays(gpu_device, *[a.ravel() for a in sample_positions(frame(p, 1), 1)])
            assert (wt == 1).all() and _same(rays, orc.camera_rays(0, 0, W, H, 1))
