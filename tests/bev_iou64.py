"""Float64 rotated-box IoU by convex clipping (test infrastructure): the intersection of two rectangles is one rectangle clipped by
the four half-planes of the other (Sutherland-Hodgman), its area the shoelace sum.  Written from the geometry, independent of the
edge-crossing + Graham-scan arithmetic of detectron2's box_iou_rotated that the kernel and the oracle restate.
Boxes are (cx, cy, w, h, angle_deg) as in detectron2: w along the rotated x axis, h along the rotated y axis."""
import math


def corners(b):
    cx, cy, w, h, a = (float(v) for v in b)
    t = math.radians(a)
    c, s = math.cos(t), math.sin(t)
    pts = []
    for dx, dy in ((-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)):  # counter-clockwise
        x, y = dx * w, dy * h
        pts.append((cx + c * x - s * y, cy + s * x + c * y))
    return pts


def _area(poly):
    a = 0.0
    for i in range(len(poly)):
        x1, y1 = poly[i]
        x2, y2 = poly[(i + 1) % len(poly)]
        a += x1 * y2 - x2 * y1
    return 0.5 * a


def _clip(poly, p, q):
    """Keep the part of `poly` left of the directed line p -> q (counter-clockwise clip edge)."""
    out = []
    side = lambda v: (q[0] - p[0]) * (v[1] - p[1]) - (q[1] - p[1]) * (v[0] - p[0])
    for i in range(len(poly)):
        a, b = poly[i], poly[(i + 1) % len(poly)]
        sa, sb = side(a), side(b)
        if sa >= 0:
            out.append(a)
        if (sa >= 0) != (sb >= 0):
            t = sa / (sa - sb)
            out.append((a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1])))
    return out


def intersection_area(b1, b2):
    poly = corners(b1)
    clip = corners(b2)
    for i in range(4):
        if not poly:
            return 0.0
        poly = _clip(poly, clip[i], clip[(i + 1) % 4])
    return abs(_area(poly)) if len(poly) >= 3 else 0.0


def iou(b1, b2):
    a1, a2 = float(b1[2]) * float(b1[3]), float(b2[2]) * float(b2[3])
    if a1 <= 0.0 or a2 <= 0.0:
        return 0.0
    inter = intersection_area(b1, b2)
    return inter / (a1 + a2 - inter)
