"""Host scene object over the C-ABI (scene_t geometry state machine + update).

Mirrors the reference's scene assembly (scene.cc:265-320,520-625) and
scene_t::update (scene.cc:748-850): meshes added in object-id order, the
kd-tree built by the host builder. No GPU is needed for anything here.
"""
import ctypes as C

import numpy as np

from . import _abi as A


class Scene:
    def __init__(self):
        self._p = C.c_void_p()
        A.check(A.lib().yk_scene_create(C.byref(self._p)))
        self.params = None
        self.instanced = False

    def __del__(self):
        try:
            if self._p:
                A.lib().yk_scene_destroy(self._p)
                self._p = C.c_void_p()
        except Exception:
            pass

    @property
    def handle(self):
        return self._p

    # -- assembly ------------------------------------------------------
    def add_material(self, type_=A.YK_MAT_SHINYDIFFUSE, color=(1, 1, 1), diffuse_reflect=None, emit=0.0,
                     power=1.0, double_sided=False, mirror_color=(1, 1, 1), specular_reflect=0.0,
                     transparency=0.0, translucency=0.0, transmit_filter=None, fresnel_effect=False, ior=None,
                     diffuse_brdf="lambert", sigma=0.1, diffuse_color=(1, 1, 1), glossy_reflect=1.0,
                     exponent=50.0, as_diffuse=True, anisotropic=False, exp_u=50.0, exp_v=50.0,
                     filter_color=(1, 1, 1), fake_shadows=False, dispersion_power=0.0):
        """shinydiffusemat / light_mat parameters with the reference factory defaults
        (shinydiffuse.cc:474-514, simple.cc:80-90); diffuse_brdf "oren_nayar"
        with roughness sigma (shinydiffuse.cc:505-514).
        type_ = A.YK_MAT_GLOSSY: glossy (glossy.cc:353-389) -- color is the gloss colour,
        diffuse_reflect defaults to 0 for it (1 for the other kinds), and
        diffuse_color, glossy_reflect, exponent, as_diffuse, anisotropic, exp_u, exp_v
        are its own; "Oren-Nayar" is accepted as the reference spells it for this kind.
        type_ = A.YK_MAT_COATED_GLOSSY: coated_glossy (coatedglossy.cc:420-498) -- the glossy
        keywords plus mirror_color and ior, which defaults to 1.4 for it (1.33 otherwise).
        type_ = A.YK_MAT_GLASS: glass (glass.cc:260-337) -- ior (default 1.4), mirror_color,
        transmit_filter (default 0 for it) and its own filter_color, fake_shadows and
        dispersion_power, which must be 0 (dispersion is not on the GPU path)."""
        brdf = {"lambert": A.YK_BRDF_LAMBERT, "oren_nayar": A.YK_BRDF_OREN_NAYAR,
                "Oren-Nayar": A.YK_BRDF_OREN_NAYAR}[diffuse_brdf]
        if diffuse_reflect is None:
            diffuse_reflect = 0.0 if type_ in (A.YK_MAT_GLOSSY, A.YK_MAT_COATED_GLOSSY) else 1.0
        if ior is None:
            ior = 1.4 if type_ in (A.YK_MAT_COATED_GLOSSY, A.YK_MAT_GLASS) else 1.33
        if transmit_filter is None:
            transmit_filter = 0.0 if type_ == A.YK_MAT_GLASS else 1.0
        m = A.yk_material(type_, A.f3(*color), diffuse_reflect, emit, power, int(double_sided),
                          A.f3(*mirror_color), specular_reflect, transparency, translucency, transmit_filter,
                          int(fresnel_effect), ior, brdf, sigma, A.f3(*diffuse_color), glossy_reflect, exponent,
                          int(as_diffuse), int(anisotropic), exp_u, exp_v)
        mid = C.c_int32()
        if type_ == A.YK_MAT_GLASS:
            g = A.yk_glass_params(A.f3(*filter_color), int(fake_shadows), dispersion_power)
            A.check(A.lib().yk_scene_add_glass(self._p, C.byref(m), C.byref(g), C.byref(mid)))
            return mid.value
        A.check(A.lib().yk_scene_add_material(self._p, C.byref(m), C.byref(mid)))
        return mid.value

    def add_mesh(self, points, faces, material):
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        fcs = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        oid = C.c_int32()
        A.check(A.lib().yk_scene_add_mesh(self._p, pts.ctypes.data_as(A.fp), len(pts),
                                          fcs.ctypes.data_as(A.i32p), len(fcs), material, C.byref(oid)))
        return oid.value

    def set_mesh_normals(self, obj_id, normals, face_normals=None, smooth=True, exported=False):
        """Vertex normals of a mesh (triangleObject_t::normals, triangle_t::na/nb/nc);
        face_normals: 3 indices per face, -1 = none (None: all missing)."""
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        fn = None if face_normals is None else np.ascontiguousarray(face_normals, dtype=np.int32).reshape(-1, 3)
        flags = (A.YK_MESH_SMOOTH if smooth else 0) | (A.YK_MESH_NORMALS_EXPORTED if exported else 0)
        A.check(A.lib().yk_scene_set_mesh_normals(self._p, obj_id, nrm.ctypes.data_as(A.fp), len(nrm),
                                                  None if fn is None else fn.ctypes.data_as(A.i32p), flags))

    def add_curve(self, points, material, strand_start=0.01, strand_end=0.01, strand_shape=0.0):
        """scene_t curve mesh (hair strand): points (n,3), n >= 2."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        oid = C.c_int32()
        A.check(A.lib().yk_scene_add_curve(self._p, pts.ctypes.data_as(A.fp), len(pts), material, strand_start,
                                           strand_end, strand_shape, C.byref(oid)))
        return oid.value

    def set_mode(self, mode):
        """scene_t::setMode: A.YK_MODE_TRIANGLE or A.YK_MODE_UNIVERSAL"""
        A.check(A.lib().yk_scene_set_mode(self._p, mode))

    def set_mesh_type(self, obj_id, type_):
        """startTriMesh's mesh type: A.YK_MESH_TRIM or A.YK_MESH_VTRIM"""
        A.check(A.lib().yk_scene_set_mesh_type(self._p, obj_id, type_))

    def set_mesh_base(self, obj_id):
        """Mark a mesh as an instancing base (not traced itself)."""
        A.check(A.lib().yk_scene_set_mesh_base(self._p, obj_id))

    def add_instance(self, base_obj_id, obj_to_world):
        """scene_t::addInstance: obj_to_world is a 4x4 row-major matrix."""
        m = np.ascontiguousarray(obj_to_world, dtype=np.float32).reshape(16)
        oid = C.c_int32()
        A.check(A.lib().yk_scene_add_instance(self._p, base_obj_id, m.ctypes.data_as(A.fp), C.byref(oid)))
        self.instanced = True
        return oid.value

    def add_area_light(self, corner, point1, point2, color=(1, 1, 1), power=1.0, samples=4):
        l = A.yk_light(A.YK_LIGHT_AREA, A.f3(*corner), A.f3(*point1), A.f3(*point2), A.f3(*color),
                       power, samples)
        A.check(A.lib().yk_scene_add_light(self._p, C.byref(l)))

    def add_point_light(self, from_, color=(1, 1, 1), power=1.0):
        """pointlight (pointlight.cc:129-139)"""
        l = A.yk_light(type=A.YK_LIGHT_POINT, color=A.f3(*color), power=power, from_=A.f3(*from_))
        A.check(A.lib().yk_scene_add_light(self._p, C.byref(l)))

    def add_directional_light(self, direction, color=(1, 1, 1), power=1.0, infinite=True, from_=(0, 0, 0),
                              radius=1.0):
        """directional (directional.cc:139-165)"""
        l = A.yk_light(type=A.YK_LIGHT_DIRECTIONAL, color=A.f3(*color), power=power, from_=A.f3(*from_),
                       direction=A.f3(*direction), radius=radius, infinite=int(infinite))
        A.check(A.lib().yk_scene_add_light(self._p, C.byref(l)))

    def add_spot_light(self, from_, to, color=(1, 1, 1), power=1.0, cone_angle=45.0, blend=0.15,
                       soft_shadows=False, samples=8, shadow_fuzzyness=1.0, photon_only=False):
        """spotlight (spotlight.cc:284-305); cone_angle is the cone's half angle in degrees"""
        l = A.yk_light(type=A.YK_LIGHT_SPOT, color=A.f3(*color), power=power, samples=samples,
                       from_=A.f3(*from_), to=A.f3(*to), cone_angle=cone_angle, blend=blend,
                       soft_shadows=int(soft_shadows), shadow_fuzzyness=shadow_fuzzyness,
                       photon_only=int(photon_only))
        A.check(A.lib().yk_scene_add_light(self._p, C.byref(l)))

    def add_sphere_light(self, from_, radius=1.0, color=(1, 1, 1), power=1.0, samples=4):
        """spherelight (spherelight.cc:196-213), without its "object" link"""
        l = A.yk_light(type=A.YK_LIGHT_SPHERE, color=A.f3(*color), power=power, samples=samples,
                       from_=A.f3(*from_), radius=radius)
        A.check(A.lib().yk_scene_add_light(self._p, C.byref(l)))

    def add_sun_light(self, direction, color=(1, 1, 1), power=1.0, angle=0.27, samples=4):
        """sunlight (sunlight.cc:115-130); angle is the half angle of the sun's disc in degrees
        (clamped to 80), carried by yk_light::cone_angle"""
        l = A.yk_light(type=A.YK_LIGHT_SUN, color=A.f3(*color), power=power, samples=samples,
                       direction=A.f3(*direction), cone_angle=angle)
        A.check(A.lib().yk_scene_add_light(self._p, C.byref(l)))

    def add_mesh_light(self, obj_ids, color=(1, 1, 1), power=1.0, samples=4, double_sided=False):
        """meshlight (meshlight.cc:221-236) over the triangles of the TRIM meshes obj_ids (one id or a
        list), concatenated in the order given"""
        ids = np.ascontiguousarray(np.atleast_1d(obj_ids), dtype=np.int32)
        l = A.yk_mesh_light(A.f3(*color), power, samples, int(double_sided))
        A.check(A.lib().yk_scene_add_mesh_light(self._p, C.byref(l), ids.ctypes.data_as(A.i32p), len(ids)))

    def mesh_light(self, i):
        """(yk_mesh_light, [object ids]) of mesh light i"""
        l, n = A.yk_mesh_light(), C.c_int32()
        A.check(A.lib().yk_scene_get_mesh_light(self._p, i, C.byref(l), None, 0, C.byref(n)))
        ids = np.zeros(max(n.value, 1), np.int32)
        A.check(A.lib().yk_scene_get_mesh_light(self._p, i, None, ids.ctypes.data_as(A.i32p), n.value, None))
        return l, [int(x) for x in ids[:n.value]]

    def mesh_light_state(self, i):
        """(yk_mesh_light_state, cdf (ntris + 1), triangle areas (ntris)) of mesh light i of a built scene"""
        st = A.yk_mesh_light_state()
        A.check(A.lib().yk_scene_get_mesh_light_state(self._p, i, C.byref(st), None, None, 0))
        cdf, areas = np.zeros(st.ntris + 1, np.float32), np.zeros(st.ntris, np.float32)
        A.check(A.lib().yk_scene_get_mesh_light_state(self._p, i, C.byref(st), cdf.ctypes.data_as(A.fp),
                                                      areas.ctypes.data_as(A.fp), st.ntris))
        return st, cdf, areas

    def set_background(self, color, power=1.0):
        """constant background (textureback.cc:206-218, ibl off), replacing a gradient one; None removes
        the constant background and leaves a gradient alone (remove_gradient_background)"""
        if color is None:
            A.check(A.lib().yk_scene_set_background(self._p, None, 0.0))
        else:
            rgb = (C.c_float * 3)(*color)
            A.check(A.lib().yk_scene_set_background(self._p, rgb, power))

    def background(self):
        """the constant background's colour (times power), or None; YkError(YK_ERR_STATE) under a gradient"""
        rgb = (C.c_float * 3)()
        has = C.c_int32()
        A.check(A.lib().yk_scene_get_background(self._p, rgb, C.byref(has)))
        return tuple(rgb) if has.value else None

    def set_gradient_background(self, horizon_color=(1, 1, 1), zenith_color=(0.4, 0.5, 1), horizon_ground_color=None,
                                zenith_ground_color=None, power=1.0):
        """gradientback (gradientback.cc:81-97) with the factory's defaults: the ground colours default
        to the sky's; replaces a constant background"""
        g = A.yk_gradient_background(A.f3(*horizon_color), A.f3(*zenith_color),
                                     A.f3(*(horizon_color if horizon_ground_color is None else horizon_ground_color)),
                                     A.f3(*(zenith_color if zenith_ground_color is None else zenith_ground_color)),
                                     power)
        A.check(A.lib().yk_scene_set_gradient_background(self._p, C.byref(g)))

    def remove_gradient_background(self):
        A.check(A.lib().yk_scene_set_gradient_background(self._p, None))

    def gradient_background(self):
        """yk_gradient_background as set, or None"""
        g = A.yk_gradient_background()
        has = C.c_int32()
        A.check(A.lib().yk_scene_get_gradient_background(self._p, C.byref(g), C.byref(has)))
        return g if has.value else None

    def add_background_light(self, samples=16, shoot_caustics=True, shoot_diffuse=True, abs_intersect=False):
        """bglight (bglight.cc:277-292; what "ibl" of a background creates): the scene's background as a
        light, appended to the light list; bound to the background at build()"""
        l = A.yk_background_light(samples, int(shoot_caustics), int(shoot_diffuse), int(abs_intersect))
        A.check(A.lib().yk_scene_add_background_light(self._p, C.byref(l)))

    def background_light_tables(self, i):
        """bgLight_t's tables of light i after build(): a dict of row_count, row_offset, row_integral,
        row_inv_integral, func_u, cdf_u, func_v, cdf_v (numpy arrays) and v_integral, v_inv_integral"""
        L = A.lib()
        nrows, total = C.c_int32(), C.c_int32()
        none = (None,) * 9
        A.check(L.yk_scene_export_background_light(self._p, i, C.byref(nrows), C.byref(total), *none))
        nv, nu = nrows.value, total.value
        t = dict(row_count=np.zeros(nv, np.int32), row_offset=np.zeros(nv, np.int32),
                 row_integral=np.zeros(nv, np.float32), row_inv_integral=np.zeros(nv, np.float32),
                 func_u=np.zeros(nu, np.float32), cdf_u=np.zeros(nu + nv, np.float32),
                 func_v=np.zeros(nv, np.float32), cdf_v=np.zeros(nv + 1, np.float32))
        vi = np.zeros(2, np.float32)
        ptr = [t[k].ctypes.data_as(A.i32p if t[k].dtype == np.int32 else A.fp) for k in
               ("row_count", "row_offset", "row_integral", "row_inv_integral", "func_u", "cdf_u", "func_v", "cdf_v")]
        A.check(L.yk_scene_export_background_light(self._p, i, None, None, *ptr, vi.ctypes.data_as(A.fp)))
        t["v_integral"], t["v_inv_integral"] = vi[0], vi[1]
        return t

    def set_camera(self, from_, to, up, resx, resy, focal=1.0, aspect_ratio=1.0, near_clip=0.0,
                   far_clip=-1.0, aperture=0.0, dof_distance=0.0, bokeh_type=0, bokeh_bias=0, bokeh_rotation=0.0,
                   type=A.YK_CAMERA_PERSPECTIVE, scale=1.0, angle=90.0, max_angle=None, circular=True,
                   mirrored=False):
        """perspectiveCam_t::factory parameters (perspectiveCamera.cc:191-232);
        bokeh_type / bokeh_bias: YK_BOKEH_* / YK_BOKEH_BIAS_*. type: YK_CAMERA_*;
        scale is the orthographic camera's, angle / max_angle (None: = angle) /
        circular / mirrored the angular one's, with the factories' defaults."""
        c = A.yk_camera(A.f3(*from_), A.f3(*to), A.f3(*up), resx, resy, focal, aspect_ratio, near_clip,
                        far_clip, aperture, dof_distance, bokeh_type, bokeh_bias, bokeh_rotation,
                        type, int(circular), int(mirrored), 0, scale, angle,
                        angle if max_angle is None else max_angle)
        A.check(A.lib().yk_scene_set_camera(self._p, C.byref(c)))

    def generate(self, name, resx, resy, p0=0, p1=0):
        """Procedural probe scenes ("cornell_dl", "cornell_pt", "bumpy"); returns render params."""
        p = A.yk_render_params()
        A.check(A.lib().yk_scene_generate(self._p, name.encode(), p0, p1, resx, resy, C.byref(p)))
        self.params = p
        return p

    # -- reference object state (what a plugin reads from live objects) ---
    def add_material_state(self, st, glass=None):
        """glass: the yk_glass_state of a YK_MAT_GLASS state (filterCol, fakeShadow)"""
        mid = C.c_int32()
        if glass is not None:
            A.check(A.lib().yk_scene_add_glass_state(self._p, C.byref(st), C.byref(glass), C.byref(mid)))
            return mid.value
        A.check(A.lib().yk_scene_add_material_state(self._p, C.byref(st), C.byref(mid)))
        return mid.value

    def glass_state(self, i):
        g = A.yk_glass_state()
        A.check(A.lib().yk_scene_get_glass_state(self._p, i, C.byref(g)))
        return g

    def add_area_light_state(self, st):
        A.check(A.lib().yk_scene_add_area_light_state(self._p, C.byref(st)))

    def set_camera_state(self, st):
        A.check(A.lib().yk_scene_set_camera_state(self._p, C.byref(st)))

    def material_states(self):
        out = []
        for k in range(self.info().nmaterials):
            m = A.yk_material_state()
            A.check(A.lib().yk_scene_get_material_state(self._p, k, C.byref(m)))
            out.append(m)
        return out

    def add_dirac_light_state(self, st):
        A.check(A.lib().yk_scene_add_dirac_light_state(self._p, C.byref(st)))

    def add_spot_light_state(self, st):
        A.check(A.lib().yk_scene_add_spot_light_state(self._p, C.byref(st)))

    def add_sphere_light_state(self, st):
        A.check(A.lib().yk_scene_add_sphere_light_state(self._p, C.byref(st)))

    def add_sun_light_state(self, st):
        A.check(A.lib().yk_scene_add_sun_light_state(self._p, C.byref(st)))

    def light_states(self):
        """Per light: yk_area_light_state, yk_dirac_light_state, yk_spot_light_state,
        yk_sphere_light_state, yk_sun_light_state, yk_background_light or yk_mesh_light_state (each getter
        answers YK_ERR_STATE for the other kinds; a mesh light's state needs a built scene)."""
        L = A.lib()
        getters = ((A.yk_area_light_state, L.yk_scene_get_area_light_state),
                   (A.yk_dirac_light_state, L.yk_scene_get_dirac_light_state),
                   (A.yk_spot_light_state, L.yk_scene_get_spot_light_state),
                   (A.yk_sphere_light_state, L.yk_scene_get_sphere_light_state),
                   (A.yk_sun_light_state, L.yk_scene_get_sun_light_state),
                   (A.yk_background_light, L.yk_scene_get_background_light),
                   (A.yk_mesh_light_state, lambda p, k, m: L.yk_scene_get_mesh_light_state(p, k, m, None, None, 0)))
        out = []
        for k in range(self.info().nlights):
            for cls, get in getters:
                m = cls()
                rc = get(self._p, k, C.byref(m))
                if rc != A.YK_ERR_STATE:
                    break
            A.check(rc)
            out.append(m)
        return out

    def camera_state(self):
        c = A.yk_camera_state()
        A.check(A.lib().yk_scene_get_camera_state(self._p, C.byref(c)))
        return c

    def build(self):
        A.check(A.lib().yk_scene_build(self._p))
        return self.info()

    # -- inspection ----------------------------------------------------
    def info(self):
        i = A.yk_scene_info()
        A.check(A.lib().yk_scene_info_get(self._p, C.byref(i)))
        return i

    def export(self):
        """Flattened prims + kd-tree as numpy arrays (the oracle's inputs)."""
        i = self.info()
        tv = np.empty((i.ntris, 9), np.float32)
        tm = np.empty(i.ntris, np.int32)
        tn = np.empty((i.ntris, 3), np.float32)
        nodes = np.empty((i.nnodes, 2), np.uint32)
        leaf = np.empty(max(i.nleaf_prims, 1), np.uint32)
        A.check(A.lib().yk_scene_export(self._p, tv.ctypes.data_as(A.fp), tm.ctypes.data_as(A.i32p),
                                        tn.ctypes.data_as(A.fp), nodes.ctypes.data_as(A.u32p),
                                        leaf.ctypes.data_as(A.u32p)))
        sm = np.empty(i.ntris, np.uint8)
        vn = np.empty((i.ntris, 9), np.float32)
        A.check(A.lib().yk_scene_export_shading(self._p, sm.ctypes.data, vn.ctypes.data_as(A.fp)))
        return dict(tri_verts=tv, tri_material=tm, tri_normal=tn, nodes=nodes, leaf_prims=leaf,
                    bound=np.array(i.bound[:], np.float32), tri_smooth=sm, tri_vnormal=vn)

    def materials(self):
        out = []
        for k in range(self.info().nmaterials):
            m = A.yk_material()
            A.check(A.lib().yk_scene_get_material(self._p, k, C.byref(m)))
            out.append(m)
        return out

    def lights(self):
        out = []
        for k in range(self.info().nlights):
            l = A.yk_light()
            A.check(A.lib().yk_scene_get_light(self._p, k, C.byref(l)))
            out.append(l)
        return out

    def camera(self):
        c = A.yk_camera()
        A.check(A.lib().yk_scene_get_camera(self._p, C.byref(c)))
        return c


def probe_scene(name, resx, resy, nu=0, nv=0):
    """Generate + build one of the BASELINE probe scenes."""
    s = Scene()
    p = s.generate(name, resx, resy, nu, nv)
    s.build()
    return s, p
