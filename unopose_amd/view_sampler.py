"""Viewpoints on a sphere around an object model, for `unopose_amd.render_train` (host, numpy, float64).

The contract is bop_toolkit_lib/view_sampler.py:sample_views -- the views a BOP `train_render` split was rendered from -- and
tests/test_render_train_cpu.py holds this module to the toolkit's own output (tests/golden/render_train_views.npz): the same views in the
same order with the same levels.  Two modes:
  hinterstoisser  the vertices of an icosahedron whose faces are split in four until there are at least `min_n_views` points (12, 42, 162,
                  642, 2562, ...), pushed onto the sphere, then ordered from the topmost point outwards: ring after ring of mesh neighbours,
                  each ring by azimuth.  A point's level is the refinement step that created it.
  fibonacci       an odd number of points of the Fibonacci lattice (an even `min_n_views` is raised by one), south to north, all of level 0.
Two properties of the toolkit are kept because files written with it depend on them:
  * the azimuth / elevation filter is a closed interval on both ends, evaluated on exactly the toolkit's float64 expressions;
  * `levels` is the level list of the UNFILTERED points.  render_train_imgs.py indexes it with the number of the view among those that
    passed the filter when it writes `view_level`, so under a restricted range a view can carry another point's level.
    `unopose_amd.render_train` does the same, so that its `scene_camera.json` equals the toolkit's.
Ring order under equal azimuths (points on a coordinate plane share one) is the order in which CPython walks the set of candidates; the rings
are therefore collected through sets filled in the toolkit's sequence, and `_ring_order` says where that matters."""
import math

import numpy as np

TWO_PI = 2.0 * math.pi
# OpenGL -> OpenCV camera axes: the rotation about x by the float pi, whose sine is 1.2e-16 and not 0 -- the toolkit's matrix, kept to the bit
_FLIP_YZ = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(math.pi), -math.sin(math.pi)], [0.0, math.sin(math.pi), math.cos(math.pi)]])


def _icosahedron():
    g = (1.0 + math.sqrt(5.0)) / 2.0
    pts = [(-1.0, g, 0.0), (1.0, g, 0.0), (-1.0, -g, 0.0), (1.0, -g, 0.0), (0.0, -1.0, g), (0.0, 1.0, g),
           (0.0, -1.0, -g), (0.0, 1.0, -g), (g, 0.0, -1.0), (g, 0.0, 1.0), (-g, 0.0, -1.0), (-g, 0.0, 1.0)]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    return pts, faces


def _split_faces(pts, levels, faces, level):
    """One refinement step: a midpoint per edge, numbered in the order the faces meet their edges (a, b), (b, c), (c, a); every face becomes
    its three corner triangles and the middle one.  Appends to `pts` and `levels`, returns the new faces."""
    midpoint, out = {}, []
    for a, b, c in faces:
        mids = []
        for i, j in ((a, b), (b, c), (c, a)):
            edge = (i, j) if i < j else (j, i)
            if edge not in midpoint:
                midpoint[edge] = len(pts)
                pts.append((0.5 * (np.array(pts[edge[0]]) + np.array(pts[edge[1]]))).tolist())
                levels.append(level)
            mids.append(midpoint[edge])
        ab, bc, ca = mids
        out += [(a, ab, ca), (ab, b, bc), (ab, bc, ca), (ca, bc, c)]
    return out


def _ring_order(pts, faces):
    """The points from the topmost one outwards: a ring is the set of not yet visited neighbours of the ring before, sorted by azimuth in
    [0, 2 pi).  The sort is stable, so points of equal azimuth stay in the set's iteration order -- which depends on the sequence of
    insertions; neighbours are therefore inserted face by face, corner by corner (next corner, then the one after), and a ring from its
    predecessor's neighbour sets in ring order, as the toolkit does."""
    neighbours = {}
    for face in faces:
        for i in range(3):
            mine = neighbours.setdefault(face[i], set())
            mine.add(face[(i + 1) % 3])
            mine.add(face[(i + 2) % 3])
    azimuth = [(math.atan2(p[1], p[0]) + TWO_PI) % TWO_PI for p in pts]
    order, seen, ring = [], [False] * len(pts), [int(np.argmax(pts[:, 2]))]
    while len(order) < len(pts):
        ring = sorted(ring, key=azimuth.__getitem__)
        reached = []
        for i in ring:
            order.append(i)
            seen[i] = True
            reached += list(neighbours[i])
        ring = [i for i in set(reached) if not seen[i]]
    return order


def hinterstoisser_points(min_n_pts, radius=1.0):
    """-> points (n,3) float64 on the sphere, n >= min_n_pts, in ring order, and their refinement levels."""
    pts, faces = _icosahedron()
    levels, level = [0] * len(pts), 0
    while len(pts) < min_n_pts:
        level += 1
        faces = _split_faces(pts, levels, faces, level)
    pts = np.array(pts)
    pts *= np.reshape(radius / np.linalg.norm(pts, axis=1), (pts.shape[0], 1))
    order = _ring_order(pts, faces)
    return pts[np.array(order), :], [levels[i] for i in order]


def fibonacci_points(n_pts, radius=1.0):
    """An odd number of points of the Fibonacci lattice, from the southernmost to the northernmost."""
    if n_pts % 2 != 1:
        raise ValueError(f"fibonacci_points: {n_pts} points (an odd number)")
    half = n_pts // 2
    turn = TWO_PI * ((math.sqrt(5.0) + 1.0) / 2.0 - 1.0)  # the complement of the golden angle
    pts = []
    for i in range(-half, half + 1):
        lat = math.asin((2 * i) / float(2 * half + 1))
        lon = (turn * i) % TWO_PI
        s = math.cos(lat) * radius
        pts.append([math.cos(lon) * s, math.sin(lon) * s, math.tan(lat) * s])
    return pts


def look_at_origin(pt):
    """Model -> camera pose (R (3,3), t (3,1)) of an OpenCV camera at `pt` that looks at the origin with the world's z axis up: gluLookAt's
    frame -- side = forward x up, or (1, 0, 0) when the camera looks along +-z and the product vanishes --, the axes flipped from OpenGL's
    to OpenCV's, t = -R pt."""
    pt = np.array(pt, np.float64)
    forward = -pt
    forward /= np.linalg.norm(forward)
    side = np.cross(forward, np.array([0.0, 0.0, 1.0]))
    if np.count_nonzero(side) == 0:
        side = np.array([1.0, 0.0, 0.0])
    side /= np.linalg.norm(side)
    up = np.cross(side, forward)
    R = _FLIP_YZ.dot(np.array([side, up, -forward]))
    return R, -R.dot(pt.reshape(3, 1))


def sample_views(min_n_views, radius=1.0, azimuth_range=(0, TWO_PI), elev_range=(-0.5 * math.pi, 0.5 * math.pi), mode="hinterstoisser"):
    """-> (views, levels): `views` a list of {"R": (3,3), "t": (3,1)} for the sampled points whose azimuth in [0, 2 pi) and elevation in
    [-pi/2, pi/2] lie inside the two CLOSED ranges, in the sampler's order; `levels` the refinement levels of ALL sampled points, filtered or
    not, in that order (see the module's note: the caller indexes it with the view number, as the toolkit's script does)."""
    if mode == "hinterstoisser":
        pts, levels = hinterstoisser_points(min_n_views, radius)
    elif mode == "fibonacci":
        pts = fibonacci_points(min_n_views + (1 - min_n_views % 2), radius)
        levels = [0] * len(pts)
    else:
        raise ValueError(f"sample_views: mode {mode!r} (hinterstoisser or fibonacci)")
    views = []
    for pt in pts:
        azimuth = math.atan2(pt[1], pt[0])
        if azimuth < 0:
            azimuth += TWO_PI
        elev = math.acos(np.linalg.norm([pt[0], pt[1], 0]) / np.linalg.norm(pt))
        if pt[2] < 0:
            elev = -elev
        if azimuth_range[0] <= azimuth <= azimuth_range[1] and elev_range[0] <= elev <= elev_range[1]:
            R, t = look_at_origin(pt)
            views.append({"R": R, "t": t})
    return views, levels
