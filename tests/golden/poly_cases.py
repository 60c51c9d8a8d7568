"""Seeded polygon inputs shared by tests/test_poly_cpu.py, tests/test_gpu_poly.py and tools/bench_poly.py."""
import numpy as np


def random_polygon(rs, h, w, kmin=3, kmax=12):
    """One polygon as a flat list [x0, y0, x1, y1, ...] of kmin..kmax vertices on an h x w image.  Coordinates are integers,
    half-integers, fifths or arbitrary doubles; a margin lets some polygons reach outside the image (negative coordinates,
    vertices beyond the right and bottom borders); the outline is star-shaped or a random vertex order (self-crossing);
    some get an exactly diagonal, a horizontal and a vertical edge, and a repeated vertex (a zero-length edge)."""
    k = int(rs.randint(kmin, kmax + 1))
    margin = float(rs.choice([0, 0, 3, max(h, w) // 4 + 1]))
    if rs.rand() < 0.5:                                                  # star-shaped around a centre
        cx, cy = rs.uniform(-margin, w + margin), rs.uniform(-margin, h + margin)
        ang = np.sort(rs.uniform(0, 2 * np.pi, size=k))
        rad = rs.uniform(0.1, 0.6, size=k) * max(h, w)
        x, y = cx + rad * np.cos(ang), cy + rad * np.sin(ang)
        x, y = np.clip(x, -margin, w + margin), np.clip(y, -margin, h + margin)
    else:
        x, y = rs.uniform(-margin, w + margin, size=k), rs.uniform(-margin, h + margin, size=k)
    grid = int(rs.randint(0, 4))
    if grid == 0:
        x, y = np.round(x), np.round(y)
    elif grid == 1:
        x, y = np.round(2 * x) / 2, np.round(2 * y) / 2
    elif grid == 2:
        x, y = np.round(5 * x) / 5, np.round(5 * y) / 5
    pts = [[float(a), float(b)] for a, b in zip(x, y)]
    if k >= 5 and rs.rand() < 0.4:                                       # diagonal, horizontal and vertical edges
        d = float(rs.randint(1, max(2, min(h, w) // 2)))
        pts[1] = [pts[0][0] + d, pts[0][1] + d]
        pts[2] = [pts[1][0] + d, pts[1][1]]
        pts[3] = [pts[2][0], pts[2][1] - 2 * d]
    if rs.rand() < 0.3:                                                  # a zero-length edge
        j = int(rs.randint(0, len(pts)))
        pts.insert(j, list(pts[j]))
    return [c for p in pts for c in p]


def random_scene(rs, h, w, n_ann, max_polys=4, kmin=3, kmax=60):
    """n_ann annotations of 1..max_polys polygons each; the second polygon of an annotation overlaps its first."""
    anns = []
    for _ in range(n_ann):
        polys = [random_polygon(rs, h, w, kmin, kmax) for _ in range(int(rs.randint(1, max_polys + 1)))]
        if len(polys) > 1:
            first = np.asarray(polys[0]).reshape(-1, 2)
            shift = np.array([rs.randint(1, 4), rs.randint(1, 4)], np.float64)
            polys[1] = [float(c) for c in (first + shift).ravel()]
        anns.append(polys)
    return anns
