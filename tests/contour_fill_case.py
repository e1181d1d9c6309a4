"""The yardstick of the contour-fill tests, written out independently of hipops/contours.py and csrc/dd_contour_fill.hip: the
definition of DESIGN 4.15 one pixel at a time in exact integer arithmetic -- a point-on-segment test for the edge pixels, even-odd
ray casting with the half-open rule for the interior -- with no scanline, no bitmap and no numpy; and a set of hand-made contours.

An `objects` list is [(label, [contour, ...]), ...] in file order, a contour a list of (x, y) integer vertices, closed implicitly."""
import functools


def _segments(contour):
    return [(contour[i], contour[(i + 1) % len(contour)]) for i in range(len(contour))]


def _on_segment(px, py, a, b):
    (x0, y0), (x1, y1) = a, b
    if (x1 - x0) * (py - y0) != (y1 - y0) * (px - x0):
        return False
    return min(x0, x1) <= px <= max(x0, x1) and min(y0, y1) <= py <= max(y0, y1)


def _crosses_at_or_left(px, py, a, b):
    """The segment counts on rows min(y0, y1) <= y < max(y0, y1), at x = x0 + (y - y0) * dx / dy: is that x <= px?"""
    (x0, y0), (x1, y1) = a, b
    if y0 == y1 or not min(y0, y1) <= py < max(y0, y1):
        return False
    dy = y1 - y0
    num = x0 * dy + (py - y0) * (x1 - x0)                      # x * dy
    return num <= px * dy if dy > 0 else num >= px * dy


def covered(px, py, contours):
    segs = [s for c in contours for s in _segments(c)]
    if any(_on_segment(px, py, a, b) for a, b in segs):
        return True
    return sum(_crosses_at_or_left(px, py, a, b) for a, b in segs) % 2 == 1


def brute_force(objects, height, width):
    """rows of the mask as a list of lists: the label of the last object that covers the pixel, 0 where none does."""
    mask = [[0] * width for _ in range(height)]
    for label, contours in objects:
        if not contours:
            continue
        xs = [x for c in contours for x, _ in c]
        ys = [y for c in contours for _, y in c]
        for py in range(max(min(ys), 0), min(max(ys), height - 1) + 1):         # nothing of the object lies outside its bounding box
            for px in range(max(min(xs), 0), min(max(xs), width - 1) + 1):
                if covered(px, py, contours):
                    mask[py][px] = label
    return mask


def _rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def _diamond(cx, cy, r):
    return [(cx, cy - r), (cx + r, cy), (cx, cy + r), (cx - r, cy)]


CANVASES = ((37, 70), (19, 130))        # (H, W): W no multiple of 32 or 64; rows cross one and two 64-bit word boundaries


def cases(height, width):
    """name -> objects; every shape fits 19 rows and lies in the 70 right-most columns, so that on the wide canvas it straddles bit 64."""
    o = width - 70
    stair = [(5, 10), (9, 6), (13, 10), (17, 6), (21, 10), (21, 14), (17, 14), (17, 16), (9, 16), (9, 14), (5, 14)]
    return {
        "border_rectangle": [(1, [_rect(0, 0, width - 1, height - 1)])],
        "diamond": [(2, [_diamond(o + 34, 9, 8)])],
        "wide_diamond_rows": [(1, [_diamond(o + 60, 9, 9)])],
        # ring, hole and island as ONE object: even-odd empties the hole and fills the island again
        "ring_hole_island": [(3, [_rect(o + 3, 1, o + 66, 17), _rect(o + 8, 4, o + 60, 14), _rect(o + 20, 7, o + 40, 11)])],
        "one_and_two_vertex_contours": [(1, [[(o + 5, 3)]]), (2, [[(o + 10, 2), (o + 25, 17)]]), (3, [[(o + 30, 5), (o + 66, 5)], [(o + 45, 8), (o + 45, 16)]]),
                                        (1, [[(o + 69, 18)], [(o + 0, 0)]])],
        # row 10 holds pass-through vertices (5,10), (21,10) and the local extremum (13,10); rows 14 and 16 hold horizontal runs between steps
        "staircase": [(2, [[(o + x, y) for x, y in stair]])],
        "staircase_reversed": [(2, [[(o + x, y) for x, y in reversed(stair)]])],
        # the second contour's top run lies on row 8, which the first contour's vertical sides cross
        "run_on_a_crossed_row": [(1, [_rect(o + 5, 3, o + 30, 12), _rect(o + 20, 8, o + 50, 15)])],
        "run_touching_a_diamond_tip": [(1, [_diamond(o + 30, 9, 6), [(o + 10, 9), (o + 24, 9)], _rect(o + 36, 9, o + 50, 12)])],
        "overlap_1_then_2": [(1, [_rect(o + 5, 2, o + 40, 12)]), (2, [_diamond(o + 40, 9, 8)])],
        "overlap_2_then_1": [(2, [_diamond(o + 40, 9, 8)]), (1, [_rect(o + 5, 2, o + 40, 12)])],
        "empty_object_between": [(1, [_rect(o + 2, 2, o + 20, 10)]), (2, []), (3, [_rect(o + 15, 6, o + 60, 16)])],
        "label_255": [(255, [_diamond(o + 20, 9, 9)]), (254, [_rect(o + 25, 0, o + 69, 18)])],
        # 60 + 10 contours: the kernel reads the records 64 at a time, the second object straddles that boundary
        "many_contours": [(1, [[(o + 1 + (7 * i) % 68, (3 * i) % 19)] for i in range(60)]),
                          (2, [_rect(o + 10, 3, o + 60, 16)] + [_rect(o + 12 + 5 * i, 5, o + 14 + 5 * i, 5 + i) for i in range(9)])],
        "no_objects": [],
    }


@functools.lru_cache(maxsize=None)
def expected(name, height, width):
    """The brute-force mask of a hand-made case as a tuple of row tuples (computed once per session, shared by the CPU and GPU tests)."""
    return tuple(tuple(r) for r in brute_force(cases(height, width)[name], height, width))
