"""Scenes whose walks fill a traversal stack to its last row (no tests here: tests/test_stack_fill_host.py pins them on the CPU, tests/test_gpu_stack_fill.py runs
them).  A stack entry is pushed only where a ray meets two or more internal children of one node, so a deep tree is not enough: the ray has to run along the
whole chain of nested boxes.  The scenes are the telescope of test_deep_trees_parity -- n triangles whose sizes and distances from the origin shrink
geometrically -- seen the other way round: camera, ray bundle and shadow rays sit at the SMALL end and look outward, the direction in which the nearer child of
every node is the one that continues, so the far ones pile up on the stack during the first descent (before any hit can cull them)."""
import dataclasses

import numpy as np

from gatling_amd.scene import CameraDesc, MaterialDesc, MeshDesc, RectLight, SceneDesc


@dataclasses.dataclass(frozen=True)
class Fill:
    name: str
    n: int           # telescope(n, ratio)
    ratio: float
    levels: int      # of the host builder's tree; bvhDepth = levels - 1 is the most entries a walk pushes
    reach: int       # the most entries the host walk (capi.bvh_stack_reach) holds over bundle(): an upper bound for any device walk of those rays
    high: int        # what the device counter must show for a render of scene(): the target of the group
    kernel: str      # the traversal kernel of a wavefront render (fused=0 for the LDS-resident ones); "k_path" runs as well where fused is 1
    rows: int        # stack rows of that variant
    fused: int       # the fused kernel takes the scene (LDS-resident, bvhDepth <= 8)
    group: int

    @property
    def depth(self):
        return self.levels - 1

    @property
    def rays_comparable(self):
        """Triangles below about 1e-7 of the scene's size: a ray within float resolution of the origin can "hit" one it misses geometrically, which no box
        test can promise to keep (test_deep_trees_parity) -- such scenes are compared by image only."""
        return self.ratio ** (-self.n) >= 1e-7


# group 1: stack 4 full; group 2: stack 8 at both ends of its range (5 and 8) and, for the lot beside a full stack, 6 and 7; group 3: LDS-resident but too deep for
# the fused kernel and k_trace; group 4: k_trace_dyn's 12 and 16 rows full; group 5: entries in the scratch spill
SCENES = (
    Fill("d4", 108, 1.05, 5, 4, 4, "k_trace", 4, 1, 1),
    Fill("d5", 92, 1.08, 6, 5, 5, "k_trace", 8, 1, 2),
    Fill("d6", 104, 1.1, 7, 6, 6, "k_trace", 8, 1, 2),
    Fill("d7", 116, 1.1, 8, 7, 7, "k_trace", 8, 1, 2),
    Fill("d8", 128, 1.1, 9, 8, 8, "k_trace", 8, 1, 2),
    Fill("d9", 116, 1.12, 10, 7, 7, "k_trace_dyn", 12, 0, 3),
    Fill("d12", 800, 1.02, 13, 12, 12, "k_trace_dyn", 12, 0, 4),
    Fill("d16", 320, 1.08, 17, 16, 16, "k_trace_dyn", 16, 0, 4),
    Fill("d22", 400, 1.1, 23, 21, 18, "k_trace_dyn", 16, 0, 5),
)
BY_NAME = {f.name: f for f in SCENES}


def unit(n, ratio):
    """The size of the telescope's largest triangle: the power of two that brings the smallest one to 0.05 .. 0.1.  A shadow ray starts at tMin = 0.01 (the
    reference's constant), so in a telescope whose small end is smaller than that no shadow walk ever enters the inner boxes; scaled by a power of two the
    tree is the same tree."""
    return float(2.0 ** np.ceil(np.log2(0.05 / ratio ** (-(n - 1)))))


def telescope_tris(n, ratio, u=None):
    """(n, 3, 3) float32 world-space triangles, scene order: triangle i has size unit * ratio^-i and lies at three times that on the x axis (the formula of
    _telescope, scaled; u = 1: that telescope itself)."""
    i = np.arange(n, dtype=np.float64)
    s = (unit(n, ratio) if u is None else u) * ratio ** (-i)
    c = np.stack([s * 3.0, 0.3 * s * ((i % 5) - 2), 0.05 * s * (i % 3)], 1)
    tri = np.array([[0, -0.5, 0], [1, 0, 0.1], [0, 0.5, 0]])
    return (c[:, None, :] + tri[None] * s[:, None, None]).astype(np.float32)


def small_end(f, u=None):
    return (unit(f.n, f.ratio) if u is None else u) * float(f.ratio ** (-(f.n - 1)))


def bundle(f, m=3000, seed=1, cone=0.45, u=None):
    """m rays from the small end outward: origins within a fifth of the smallest triangle's distance of the origin, directions in a cone about +x."""
    rng = np.random.default_rng(seed)
    o = (rng.uniform(-1, 1, (m, 3)) * (3.0 * small_end(f, u)) * 0.2).astype(np.float32)
    th = rng.uniform(0, cone, m); ph = rng.uniform(0, 2 * np.pi, m)
    d = np.stack([np.cos(th), np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph)], 1).astype(np.float32)
    return o, d


def scene(f, material=None, light=False, zc=-0.3, zl=(0.28, 0.40)):
    """The telescope with its camera at the small end, `zc` sizes of the smallest triangle below the triangles' plane, looking outward and slightly up at their
    undersides (every triangle rises towards the big end, so it is the undersides that face a light there).  From -0.3 the camera rays ALONE reach the target
    row in every scene (counted: test_gpu_stack_fill.test_aovs_against_the_oracle); from -0.6 those of the bvhDepth-8 scene stop a row short.  `light`: a
    rectangle at the big end that faces the small end, at the height `zl` from which shadow rays run along the whole chain of boxes."""
    from gatling_amd.meshprep import bake_vertices
    p = telescope_tris(f.n, f.ratio).reshape(-1, 3)
    q = p.astype(np.float64)  # (the squares of the largest scene's coordinates overflow fp32)
    nrm = np.cross(q[1::3] - q[0::3], q[2::3] - q[0::3]); nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    s = small_end(f)
    desc = SceneDesc(meshes=[MeshDesc("telescope", bake_vertices(p, np.repeat(nrm.astype(np.float32), 3, axis=0)), np.arange(3 * f.n, dtype=np.uint32).reshape(-1, 3), 0,
                                      double_sided=True)],
                     materials=[material if material is not None else MaterialDesc.usd_preview_surface(diffuseColor=(0.8, 0.7, 0.6), roughness=0.5)],
                     camera=CameraDesc(position=(0.0, 0.0, zc * s), forward=(1.0, 0.0, 0.02), up=(0, 0, 1), vfov=0.9, clip_start=0.0, clip_end=1.0e30))
    if light:
        # Seen from the small end every triangle spans the slopes z / x = 0 .. 0.05 and every box 0 .. 0.067 or more; a shadow ray that rises at 0.06 .. 0.09
        # passes over the triangles of every larger size while it is still inside their boxes, so it is not ended by an occluder in an upper node (an any-hit
        # walk ends at its first hit) before it has descended the whole chain.  The light spans those slopes at x = 4.5.
        u = unit(f.n, f.ratio)
        desc.rect_lights.append(RectLight(origin=(4.5 * u, 0.0, 0.5 * (zl[0] + zl[1]) * u), t0=(0, 1, 0), t1=(0, 0, 1), base_emission=(9, 9, 9), width=2.0 * u,
                                          height=(zl[1] - zl[0]) * u))
    return desc


def scene_tris(desc):
    """World-space triangles of a scene in scene order, as the host builder sees them."""
    tris = []
    for m in desc.meshes:
        p = np.asarray(m.vertices)["pos"].reshape(-1, 3).astype(np.float64)
        p = (np.concatenate([p, np.ones((len(p), 1))], axis=1) @ np.asarray(m.transform, np.float64).reshape(4, 4))[:, :3]
        tris.append(p[np.asarray(m.faces, np.int64).reshape(-1)])
    return np.ascontiguousarray(np.concatenate(tris), np.float32).reshape(-1, 3, 3)
