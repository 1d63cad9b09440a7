"""Constructed response planes for the detection chain at its edges (tests/test_detect_edges.py).

Plain numpy, seeded, no files, no GPU.  The planes of one octave - blur L[5] and response R[5], each rows x cols - are zero
everywhere (below both thresholds: nothing fires) except for isolated SITES: small stencils written into R[level .. level+2]
(low, cur, high of findLevelKeypoints, pyramid.cpp:206-222) and into L[level+1] (getHessianPointType's plane) around a chosen
(level, r0, c0).  The frame of every R plane (row and column 0 and n-1) is large finite garbage which nothing may use.

A site = a STENCIL (what localizeKeypoint, pyramid.cpp:122-204, makes of it: how often the centre moves, where to, how it
leaves) x a POSITION (where the extrema scan k_extrema_march and k_localize meet it: strip and lane seams, band seams, first
and last scanned row and column, the frame).  Every site carries a CLAIM - candidate or not, the centre of every iteration,
the exit, kept or dropped, and for some the very bits of b, val or edgeScore; the CPU half of the tests proves each claim with
the oracle's trace, so the inputs cannot rot, and the GPU half compares the chain's output with the oracle's kept list.

Stencil values are small integers x 32 (exact in float32 and in every difference the chain takes of them), hand-derived where
a few lines of algebra give them and otherwise found by a seeded search against the oracle and written down here.  Moves: the
first centre is a 27-neighbour extremum, so along one axis alone its offset is at most 0.5; the searched stencils get their first
move from the dxs coupling (a large negative `low` neighbour).  Searched stencils are one row tall: the rows above and below are
zero, which decouples y (dy = dxy = dys = 0, b[1] = +-0 exactly); their transposes decouple x.

Spacing: the box of a site - its cells and every centre of its path - is at least 3 pixels from the box of any other, in rows or in
columns (checked by `build`): a centre reads one pixel around itself, so no value of one site is in reach of a centre of another -
except where a collision is meant.  (The positions themselves - four adjacent columns of a lane, both sides of a seam - are closer to
each other than 8 pixels; such sites sit in different rows.)
"""
import numpy as np

F = np.float32
BORDER = 5                 # pyramid.h:39
U = F(32.0)                # one stencil unit
V = 8                      # the searched stencils' first centre, in units

# exits of localizeKeypoint, numbered like the oracle's TraceExit
KEPT, EDGE_HIGH, EDGE_NEG, NAN, OUT_RIGHT, OUT_DOWN, OUT_LEFT, OUT_UP, SHIFT, WEAK, TAKEN = range(11)

# the two parameter sets of the GPU half (one context each)
PSETS = {"default": {}, "ratio4": dict(threshold=2.5, edgeEigenValueRatio=4.0)}


def bits(v):
    return int(np.array([v], F).view(np.uint32)[0])


def from_bits(u):
    return np.array([u], np.uint32).view(F)[0]


def step(v, n):
    """the float32 n steps above (n < 0: below) the finite non-zero float32 v, in the order of the real numbers"""
    u = bits(v)
    return from_bits(u + n if v > 0 else u - n)


def thresholds(pset):
    """(positiveThreshold, finalThreshold, edgeScoreThreshold) as pyramid.h:59-64 computes them in float32"""
    kw = PSETS[pset]
    t = F(kw.get("threshold", F(16.0) / F(3.0))); r = F(kw.get("edgeEigenValueRatio", 10.0))
    final = F(t * t)
    return F(0.8 * float(final)), final, F(F((r + F(1)) * (r + F(1))) / r)


# ----------------------------------------------------------------------------------------------------------------------
# Stencils: cells {(p, dr, dc): units}, p = 0, 1, 2 = low, cur, high (3 = the plane above high, for two-level stencils), relative
# to the first centre.  `path` = the centres of the iterations relative to it, `exit` = how localizeKeypoint leaves when no
# border is in the way.
# ----------------------------------------------------------------------------------------------------------------------
SEARCHED = {'b0_06_above': {'bits_at': ((0, 1), 0, 1058642330),
                 'cells': {(0, 0, -1): 7,
                           (0, 0, 1): -4,
                           (0, 0, 2): 13,
                           (1, 0, -1): -6,
                           (1, 0, 0): 8,
                           (1, 0, 1): 7,
                           (1, 0, 2): 7,
                           (2, 0, -1): -24,
                           (2, 0, 0): 4,
                           (2, 0, 1): 1,
                           (2, 0, 2): 10},
                 'exit': 0,
                 'path': [(0, 0), (0, 1), (0, 2)]},
 'b0_06_below': {'bits_at': ((0, 1), 0, 1058642329),
                 'cells': {(0, 0, -1): 7,
                           (0, 0, 1): -4,
                           (0, 0, 2): 13,
                           (1, 0, -1): -6,
                           (1, 0, 0): 8,
                           (1, 0, 1): 7,
                           (1, 0, 2): 7,
                           (2, 0, -1): -24,
                           (2, 0, 0): 4,
                           (2, 0, 1): 1,
                           (2, 0, 2): 10},
                 'exit': 0,
                 'path': [(0, 0), (0, 1)]},
 'b0_15': {'bits': {'b0': 1069547520},
           'cells': {(0, 0, -1): 3,
                     (0, 0, 0): 3,
                     (0, 0, 1): 7,
                     (0, 0, 2): 0,
                     (0, 0, 3): -14,
                     (0, 0, 4): -20,
                     (0, 0, 5): -21,
                     (1, 0, -1): -4,
                     (1, 0, 0): 8,
                     (1, 0, 1): 6,
                     (1, 0, 2): 4,
                     (1, 0, 3): 21,
                     (1, 0, 4): 23,
                     (1, 0, 5): 24,
                     (2, 0, -1): 6,
                     (2, 0, 0): -14,
                     (2, 0, 1): -24,
                     (2, 0, 2): 14,
                     (2, 0, 3): -6,
                     (2, 0, 4): -11,
                     (2, 0, 5): -13},
           'exit': 0,
           'path': [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4)]},
 'b0_15_above': {'bits_at': ((0, 4), 0, 1069547521),
                 'cells': {(0, 0, -1): 3,
                           (0, 0, 0): 3,
                           (0, 0, 1): 7,
                           (0, 0, 2): 0,
                           (0, 0, 3): -14,
                           (0, 0, 4): -20,
                           (1, 0, -1): -4,
                           (1, 0, 0): 8,
                           (1, 0, 1): 6,
                           (1, 0, 2): 4,
                           (1, 0, 3): 21,
                           (1, 0, 4): 23,
                           (1, 0, 5): 24,
                           (2, 0, -1): 6,
                           (2, 0, 0): -14,
                           (2, 0, 1): -24,
                           (2, 0, 2): 14,
                           (2, 0, 3): -6,
                           (2, 0, 4): -11,
                           (2, 0, 5): -13},
                 'exit': 8,
                 'path': [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4)]},
 'b1_06_above': {'bits_at': ((1, 0), 1, 1058642330),
                 'cells': {(0, -1, 0): 7,
                           (0, 1, 0): -4,
                           (0, 2, 0): 13,
                           (1, -1, 0): -6,
                           (1, 0, 0): 8,
                           (1, 1, 0): 7,
                           (1, 2, 0): 7,
                           (2, -1, 0): -24,
                           (2, 0, 0): 4,
                           (2, 1, 0): 1,
                           (2, 2, 0): 10},
                 'exit': 0,
                 'path': [(0, 0), (1, 0), (2, 0)]},
 'b1_06_below': {'bits_at': ((1, 0), 1, 1058642329),
                 'cells': {(0, -1, 0): 7,
                           (0, 1, 0): -4,
                           (0, 2, 0): 13,
                           (1, -1, 0): -6,
                           (1, 0, 0): 8,
                           (1, 1, 0): 7,
                           (1, 2, 0): 7,
                           (2, -1, 0): -24,
                           (2, 0, 0): 4,
                           (2, 1, 0): 1,
                           (2, 2, 0): 10},
                 'exit': 0,
                 'path': [(0, 0), (1, 0)]},
 'b1_15_above': {'bits_at': ((4, 0), 1, 1069547521),
                 'cells': {(0, -1, 0): 3,
                           (0, 0, 0): 3,
                           (0, 1, 0): 7,
                           (0, 2, 0): 0,
                           (0, 3, 0): -14,
                           (0, 4, 0): -20,
                           (1, -1, 0): -4,
                           (1, 0, 0): 8,
                           (1, 1, 0): 6,
                           (1, 2, 0): 4,
                           (1, 3, 0): 21,
                           (1, 4, 0): 23,
                           (1, 5, 0): 24,
                           (2, -1, 0): 6,
                           (2, 0, 0): -14,
                           (2, 1, 0): -24,
                           (2, 2, 0): 14,
                           (2, 3, 0): -6,
                           (2, 4, 0): -11,
                           (2, 5, 0): -13},
                 'exit': 8,
                 'path': [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0)]},
 'b2_15': {'bits': {'b2': 1069547520},
           'cells': {(0, 0, -1): -18,
                     (0, 0, 0): 8,
                     (0, 0, 1): 7,
                     (0, 0, 2): 0,
                     (1, 0, -1): -14,
                     (1, 0, 0): 8,
                     (1, 0, 1): 5,
                     (1, 0, 2): -5,
                     (2, 0, -1): -2,
                     (2, 0, 0): 3,
                     (2, 0, 1): 2,
                     (2, 0, 2): 23},
           'exit': 0,
           'path': [(0, 0), (0, 1)]},
 'b2_15_above': {'bits_at': ((0, 1), 2, 1069547521),
                 'cells': {(0, 0, -1): -18,
                           (0, 0, 0): 8,
                           (0, 0, 2): 0,
                           (1, 0, -1): -14,
                           (1, 0, 0): 8,
                           (1, 0, 1): 5,
                           (1, 0, 2): -5,
                           (2, 0, -1): -2,
                           (2, 0, 0): 3,
                           (2, 0, 1): 2,
                           (2, 0, 2): 23},
                 'exit': 8,
                 'path': [(0, 0), (0, 1)]},
 'chain1': {'cells': {(0, 0, -1): -9,
                      (0, 0, 0): -2,
                      (0, 0, 1): -3,
                      (0, 0, 2): 1,
                      (1, 0, -1): -7,
                      (1, 0, 0): 8,
                      (1, 0, 1): 8,
                      (1, 0, 2): -19,
                      (2, 0, -1): -19,
                      (2, 0, 0): 7,
                      (2, 0, 1): 1,
                      (2, 0, 2): 19},
            'exit': 0,
            'path': [(0, 0), (0, 1)]},
 'chain2': {'cells': {(0, 0, -1): -10,
                      (0, 0, 0): 2,
                      (0, 0, 1): 8,
                      (0, 0, 2): 8,
                      (0, 0, 3): -7,
                      (1, 0, -1): -1,
                      (1, 0, 0): 8,
                      (1, 0, 1): 7,
                      (1, 0, 2): 8,
                      (1, 0, 3): 24,
                      (2, 0, -1): 3,
                      (2, 0, 0): -5,
                      (2, 0, 1): -10,
                      (2, 0, 2): 23,
                      (2, 0, 3): -13},
            'exit': 0,
            'path': [(0, 0), (0, 1), (0, 2)]},
 'chain3': {'cells': {(0, 0, -1): 0,
                      (0, 0, 0): -3,
                      (0, 0, 1): -9,
                      (0, 0, 2): 20,
                      (0, 0, 3): -1,
                      (0, 0, 4): 16,
                      (1, 0, -1): -1,
                      (1, 0, 0): 8,
                      (1, 0, 1): 8,
                      (1, 0, 2): 7,
                      (1, 0, 3): -3,
                      (1, 0, 4): -4,
                      (2, 0, -1): -7,
                      (2, 0, 0): 6,
                      (2, 0, 1): 5,
                      (2, 0, 2): -18,
                      (2, 0, 3): -22,
                      (2, 0, 4): -24},
            'exit': 0,
            'path': [(0, 0), (0, 1), (0, 2), (0, 3)]},
 'chain4': {'cells': {(0, 0, -1): -3,
                      (0, 0, 0): -6,
                      (0, 0, 1): -21,
                      (0, 0, 2): 8,
                      (0, 0, 3): -19,
                      (0, 0, 4): -19,
                      (0, 0, 5): -22,
                      (1, 0, -1): -17,
                      (1, 0, 0): 8,
                      (1, 0, 1): 7,
                      (1, 0, 2): 5,
                      (1, 0, 3): 7,
                      (1, 0, 4): -12,
                      (1, 0, 5): 3,
                      (2, 0, -1): -19,
                      (2, 0, 0): 6,
                      (2, 0, 1): -5,
                      (2, 0, 2): -21,
                      (2, 0, 3): 19,
                      (2, 0, 4): 13,
                      (2, 0, 5): 9},
            'exit': 0,
            'path': [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4)]},
 'diag': {'cells': {(0, -1, 0): -8,
                    (0, 0, -1): -13,
                    (0, 0, 0): -8,
                    (0, 0, 1): -17,
                    (0, 1, 0): -23,
                    (0, 1, 1): -21,
                    (0, 1, 2): -10,
                    (0, 2, 1): 1,
                    (1, -1, -1): 1,
                    (1, -1, 0): -22,
                    (1, -1, 1): -18,
                    (1, 0, -1): -4,
                    (1, 0, 0): 8,
                    (1, 0, 1): 8,
                    (1, 0, 2): -3,
                    (1, 1, -1): -1,
                    (1, 1, 0): 6,
                    (1, 1, 1): 7,
                    (1, 1, 2): -10,
                    (1, 2, 0): -9,
                    (1, 2, 1): 8,
                    (1, 2, 2): 13,
                    (2, -1, 0): -3,
                    (2, 0, -1): 7,
                    (2, 0, 0): 2,
                    (2, 0, 1): -15,
                    (2, 1, 0): -7,
                    (2, 1, 1): -12,
                    (2, 1, 2): 11,
                    (2, 2, 1): 15},
          'exit': 0,
          'path': [(0, 0), (1, 1)]},
 'loserneighbour': {'cells': {(0, 0, -1): 0,
                              (0, 0, 0): -17,
                              (0, 0, 1): -4,
                              (0, 0, 2): -17,
                              (0, 0, 3): 0,
                              (1, 0, -1): -2,
                              (1, 0, 0): 8,
                              (1, 0, 1): 7,
                              (1, 0, 2): 8,
                              (1, 0, 3): -2,
                              (2, 0, -1): -8,
                              (2, 0, 0): 8,
                              (2, 0, 1): 6,
                              (2, 0, 2): 8,
                              (2, 0, 3): -8,
                              (3, 0, 1): -2,
                              (3, 0, 2): -19,
                              (3, 0, 3): -5},
                    'exit': 0,
                    'others': [(0, 0, 2, [(0, 2), (0, 1)], 10), (1, 0, 2, [(0, 2)], 0)],
                    'path': [(0, 0), (0, 1)]},
 'lowerwins': {'anchor': (0, 1),
               'cells': {(0, 0, -1): -14,
                         (0, 0, 0): -15,
                         (0, 0, 1): 6,
                         (0, 0, 2): -9,
                         (1, 0, -1): -22,
                         (1, 0, 0): 7,
                         (1, 0, 1): 8,
                         (1, 0, 2): -1,
                         (2, 0, -1): 0,
                         (2, 0, 0): 8,
                         (2, 0, 1): 1,
                         (2, 0, 2): -20,
                         (3, 0, -1): 7,
                         (3, 0, 0): -22,
                         (3, 0, 1): -11,
                         (3, 0, 2): -21},
               'exit': 0,
               'others': [(1, 0, 0, [(0, 0)], 10)],
               'path': [(0, 1), (0, 0)]},
 'near06': {'cells': {(0, 0, -1): 7,
                      (0, 0, 0): -9,
                      (0, 0, 1): -4,
                      (0, 0, 2): 13,
                      (1, 0, -1): -6,
                      (1, 0, 0): 8,
                      (1, 0, 1): 7,
                      (1, 0, 2): 7,
                      (2, 0, -1): -24,
                      (2, 0, 0): 4,
                      (2, 0, 1): 1,
                      (2, 0, 2): 10},
            'exit': 0,
            'path': [(0, 0), (0, 1)]},
 'pair': {'cells': {(0, 0, -1): 0,
                    (0, 0, 0): -17,
                    (0, 0, 1): -4,
                    (0, 0, 2): -17,
                    (0, 0, 3): 0,
                    (1, 0, -1): -2,
                    (1, 0, 0): 8,
                    (1, 0, 1): 7,
                    (1, 0, 2): 8,
                    (1, 0, 3): -2,
                    (2, 0, -1): -17,
                    (2, 0, 0): -1,
                    (2, 0, 1): 5,
                    (2, 0, 2): -1,
                    (2, 0, 3): -17},
          'exit': 0,
          'others': [(0, 0, 2, [(0, 2), (0, 1)], 10)],
          'path': [(0, 0), (0, 1)]},
 'still5': {'cells': {(0, 0, -1): 7,
                      (0, 0, 0): -23,
                      (0, 0, 1): -17,
                      (0, 0, 2): -20,
                      (0, 0, 3): 2,
                      (0, 0, 4): 14,
                      (0, 0, 5): 19,
                      (1, 0, -1): -7,
                      (1, 0, 0): 8,
                      (1, 0, 1): 8,
                      (1, 0, 2): 4,
                      (1, 0, 3): 9,
                      (1, 0, 4): -3,
                      (1, 0, 5): -7,
                      (2, 0, -1): -19,
                      (2, 0, 0): -16,
                      (2, 0, 1): 8,
                      (2, 0, 2): 22,
                      (2, 0, 3): 12,
                      (2, 0, 4): 19,
                      (2, 0, 5): 23},
            'exit': 0,
            'path': [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4)]},
 'threeway': {'cells': {(0, 0, -1): 0,
                        (0, 0, 0): -17,
                        (0, 0, 1): -4,
                        (0, 0, 2): -17,
                        (0, 0, 3): 0,
                        (1, 0, -1): -2,
                        (1, 0, 0): 8,
                        (1, 0, 1): 7,
                        (1, 0, 2): 8,
                        (1, 0, 3): -2,
                        (2, 0, -1): -18,
                        (2, 0, 0): -1,
                        (2, 0, 1): 8,
                        (2, 0, 2): -1,
                        (2, 0, 3): -18,
                        (3, 0, 0): -13,
                        (3, 0, 1): -16,
                        (3, 0, 2): -1},
              'exit': 0,
              'others': [(0, 0, 2, [(0, 2), (0, 1)], 10), (1, 0, 1, [(0, 1)], 10)],
              'path': [(0, 0), (0, 1)]}}

# tuned cells: a float32 bit pattern (of the value itself, not of units) replaces a cell of a searched stencil
TUNED = {'b0_06_above': {(0, 0, 0): 3276262366},
 'b0_06_below': {(0, 0, 0): 3276262375},
 'b0_15_above': {(0, 0, 5): 3290955779},
 'b1_06_above': {(0, 0, 0): 3276262366},
 'b1_06_below': {(0, 0, 0): 3276262375},
 'b1_15_above': {(0, 5, 0): 3290955779},
 'b2_15_above': {(0, 0, 1): 1130364927}}

# How far the 0.6 sites' b got from the double 0.6 and the 1.5 sites' b from 1.5: name -> (bits of b, steps).  Steps count float32
# values from the constant towards b, the first float32 on that side being step 1 (0.6 is no float32: 0x3f199999 < 0.6 < 0x3f19999a;
# 1.5 is one: 0x3fc00001 is its step 1).  Every site reached step 1, the adjacent float32.
REACHED = {'b0_06_above': (1058642330, 1),
 'b0_06_below': (1058642329, 1),
 'b0_15_above': (1069547521, 1),
 'b1_06_above': (1058642330, 1),
 'b1_06_below': (1058642329, 1),
 'b1_15_above': (1069547521, 1),
 'b2_15_above': (1069547521, 1)}


class Stencil:
    def __init__(self, name, cells, path, exit_, lcells=None, bits_=None, others=(), tuned=None):
        self.name = name
        self.cells = {k: (v if isinstance(v, np.float32) else F(F(v) * U)) for k, v in cells.items()}   # float32 values
        for k, u in (tuned or {}).items():
            self.cells[k] = from_bits(u)
        self.path = list(path)        # [(dr, dc)] of every iteration; [] = no candidate
        self.exit = exit_
        self.lcells = dict(lcells or {})   # {(dr, dc): float32} of L[level + 1]
        self.bits = dict(bits_ or {})      # claimed bits: "b0", "b1", "b2", "val", "edge" -> uint32
        self.others = list(others)         # further claimed candidates of this stencil: (dlevel, dr, dc, path, exit)
        self.bits_at = None                # ((dr, dc), k, uint32): b[k] of the iteration whose centre is (dr, dc)
        self.type = None                   # claimed type of a kept site (0, 1; 2 = negative response)

    def _map(self, name, fn, exit_map):
        s = Stencil.__new__(Stencil)
        s.name = name
        s.cells = {(p,) + fn(dr, dc): v for (p, dr, dc), v in self.cells.items()}
        s.path = [fn(*q) for q in self.path]
        s.exit = exit_map.get(self.exit, self.exit)
        s.lcells = {fn(*k): v for k, v in self.lcells.items()}
        s.bits = dict(self.bits)
        s.type = self.type
        s.bits_at = None if self.bits_at is None else (fn(*self.bits_at[0]),) + tuple(self.bits_at[1:])
        s.others = [(dl,) + fn(dr, dc) + ([fn(*q) for q in pth], exit_map.get(ex, ex)) for dl, dr, dc, pth, ex in self.others]
        return s

    def mirrored(self):
        """columns reversed: b[0] changes its sign and nothing else changes (IEEE arithmetic is symmetric in the sign)"""
        s = self._map(self.name + ":mirror", lambda dr, dc: (dr, -dc), {OUT_RIGHT: OUT_LEFT, OUT_LEFT: OUT_RIGHT})
        if "b0" in s.bits:
            s.bits["b0"] ^= 0x80000000
        if s.bits_at is not None and s.bits_at[1] == 0:
            s.bits_at = (s.bits_at[0], 0, s.bits_at[2] ^ 0x80000000)
        return s

    def mirrored_rows(self):
        """rows reversed: b[1] changes its sign"""
        s = self._map(self.name + ":mirror_rows", lambda dr, dc: (-dr, dc), {OUT_DOWN: OUT_UP, OUT_UP: OUT_DOWN})
        if "b1" in s.bits:
            s.bits["b1"] ^= 0x80000000
        if s.bits_at is not None and s.bits_at[1] == 1:
            s.bits_at = (s.bits_at[0], 1, s.bits_at[2] ^ 0x80000000)
        return s

    def transposed(self):
        """rows and columns exchanged (the solve is not symmetric in them: a transposed stencil's bits are its own)"""
        s = self._map(self.name + ":transpose", lambda dr, dc: (dc, dr), {OUT_RIGHT: OUT_DOWN, OUT_DOWN: OUT_RIGHT, OUT_LEFT: OUT_UP, OUT_UP: OUT_LEFT})
        s.bits = {{"b0": "b1", "b1": "b0"}.get(k, k): v for k, v in self.bits.items()}
        if s.bits_at is not None:
            s.bits_at = (s.bits_at[0], {0: 1, 1: 0}.get(s.bits_at[1], 2), s.bits_at[2])
        return s

    def negated(self):
        """every value negated: the mirror image in the sign (minima for maxima), every b the same, val negated"""
        s = self._map(self.name + ":neg", lambda dr, dc: (dr, dc), {})
        s.cells = {k: F(-v) for k, v in s.cells.items()}
        if "val" in s.bits:
            s.bits["val"] ^= 0x80000000
        return s

    def cut(self, dc_max):
        """without the cells right of dc_max and the path beyond it: for a chain whose last centres lie behind a border test"""
        s = self._map(self.name + ":cut", lambda dr, dc: (dr, dc), {})
        s.cells = {k: v for k, v in s.cells.items() if k[2] <= dc_max}
        return s

    def with_l(self, name, lcells):
        s = self._map(self.name + ":" + name, lambda dr, dc: (dr, dc), {})
        s.lcells = dict(lcells)
        return s

    def box(self):
        """rows and columns of the cells and of the centres (a centre outside the cells is never reached: Stencil.cut)"""
        r_lo = min(k[1] for k in self.cells); r_hi = max(k[1] for k in self.cells)
        c_lo = min(k[2] for k in self.cells); c_hi = max(k[2] for k in self.cells)
        rs = [k[0] for k in self.lcells] + [q[0] for q in self.path if r_lo <= q[0] <= r_hi and c_lo <= q[1] <= c_hi]
        cs = [k[1] for k in self.lcells] + [q[1] for q in self.path if r_lo <= q[0] <= r_hi and c_lo <= q[1] <= c_hi]
        return min(rs + [r_lo]), max(rs + [r_hi]), min(cs + [c_lo]), max(cs + [c_hi])


def peak(value, name="peak"):
    """the zero-gradient site: one pixel, zeros around: dx = dy = ds = 0, b = -0/.. = 0, val == the pixel, edgeScore 4"""
    return Stencil(name, {(1, 0, 0): F(value)}, [(0, 0)], KEPT, bits_={"val": bits(F(value)), "edge": bits(F(4.0))})


def cross(k, v, up_steps=0, left_steps=0, name="cross"):
    """dxx = -4k, dyy = -k, dxy = 0: edgeScore = 25 k^2 / 4 k^2 = 6.25 exactly, the threshold of edgeEigenValueRatio = 4.
    up_steps / left_steps move the upper / left neighbour by float32 steps: the score then leaves 6.25 (CROSS_NEAR)."""
    k = F(k); v = F(v)
    a = F(v - F(2) * k); b = F(v - k / F(2))
    up = step(b, up_steps) if up_steps else b
    left = step(a, left_steps) if left_steps else a
    return Stencil(name, {(1, 0, 0): v, (1, 0, -1): left, (1, 0, 1): a, (1, -1, 0): up, (1, 1, 0): b}, [(0, 0)], KEPT)


# (up_steps, left_steps) of the crosses (k = 16, v = 64) whose score is the float32 next to 6.25 on either side (found by trying -6 .. 6)
CROSS_NEAR = {"below": (-2, -6), "above": (-1, -5)}


def plateau(v):
    """all nine `cur` values equal, low and high not above: the centre's edgeScore is 0/0 = NaN, which passes both comparisons
    (pyramid.cpp:145) and dies at the NaN test after the solve.  The eight rim pixels are candidates too: the four edge
    pixels have dxx = -v or dyy = -v, the other +0 and dxy = 0: the determinant is (-v)(+0) - 0 = -0 and the score v^2 / -0 =
    -inf, which leaves by `edgeScore < 0`."""
    cells = {(1, r, c): F(v) for r in (-1, 0, 1) for c in (-1, 0, 1)}
    rim = [(0, 0, -1, [(0, -1)], EDGE_NEG), (0, 0, 1, [(0, 1)], EDGE_NEG), (0, -1, 0, [(-1, 0)], EDGE_NEG), (0, 1, 0, [(1, 0)], EDGE_NEG)]
    return Stencil("plateau", cells, [(0, 0)], NAN, others=rim)


def plateau_min(v):
    """the plateau of minima: the rim's determinant is (+v)(+0) - 0 = +0 and its score v^2 / +0 = +inf: `edgeScore >= threshold`"""
    st = plateau(v).negated()
    st.others = [(dl, dr, dc, pth, EDGE_HIGH) for dl, dr, dc, pth, ex in st.others]
    return st


def saddle(v):
    """a saddle that is still a 27-neighbour maximum through ties: left and right equal the centre (dxx = 0), one corner is
    non-zero (dxy = v / 4): the determinant -dxy^2 is negative and so is the score"""
    v = F(v)
    return Stencil("saddle", {(1, 0, -1): v, (1, 0, 0): v, (1, 0, 1): v, (1, 1, 1): v}, [(0, 0)], EDGE_NEG)


def ties(offsets, v, name, exits=None):
    """adjacent equal maxima: every one of them is a candidate (isMax rejects only a GREATER neighbour, pyramid.cpp:39-48) and rests on
    its own pixel; exits[i]: how the i-th leaves (kept, but for the middle of three in a row or column: dxx or dyy = 0 there and the
    corners make no dxy, so its score is 4 v^2 / -0 < 0)"""
    cells = {(1, dr, dc): F(v) for dr, dc in offsets}
    exits = exits or [KEPT] * len(offsets)
    return Stencil(name, cells, [(0, 0)], exits[0], others=[(0, dr, dc, [(dr, dc)], ex) for (dr, dc), ex in zip(offsets[1:], exits[1:])])


def two_levels(v):
    """R[l+1] == R[l+2] in the whole neighbourhood: the same pixel is a candidate at two levels, both rest on it, and the
    octaveMap - one per octave, not per level (pyramid.cpp:226) - keeps the lower one"""
    v = F(v)
    return Stencil("two_levels", {(1, 0, 0): v, (2, 0, 0): v}, [(0, 0)], KEPT, others=[(1, 0, 0, [(0, 0)], TAKEN)])


# The pivot sites (found by a seeded search against the oracle): the first centre's system has a tie in one comparison of solveLinear3x3
# (helpers.cpp:49-53 `tmp > vp`, `fabsf(A[6]) > vp`; :64 `fabsf(A[4]) < fabsf(A[7])`), it is regular, the site rests where it is and
# is kept with the b recorded here - and solve3x3 with that comparison decided the other way gives another b (the CPU tests show both).
#    xy     |dxx| == |dxy| > |dxs|: `tmp > vp` at equality.  (dxy^2 = dxx^2 makes the score at least 8: under edgeEigenValueRatio = 4
#    ys_gt  |dxy| == |dxs| > |dxx|: `fabsf(A[6]) > vp` at equality, row 1 being the pivot.     these two leave at the edge test)
#    xs     |dxx| == |dxs| > |dxy|: `fabsf(A[6]) > vp` at equality, row 0 being the pivot
#    a47    |a4| == |a7| after the elimination, no tie in the first search
PIVOT_FLIP = {"xy": "first", "xs": "second", "ys_gt": "second", "a47": "third"}
PIVOT = {'a47': {'bits': {'b0': 3199136706, 'b1': 3174682199, 'b2': 3183595817},
         'cells': {(0, -1, 0): -2,
                   (0, 0, -1): -11,
                   (0, 0, 0): -2,
                   (0, 0, 1): -3,
                   (0, 1, 0): -16,
                   (1, -1, -1): 1,
                   (1, -1, 0): 4,
                   (1, -1, 1): -4,
                   (1, 0, -1): 7,
                   (1, 0, 0): 8,
                   (1, 0, 1): -2,
                   (1, 1, -1): -20,
                   (1, 1, 0): 6,
                   (1, 1, 1): -9,
                   (2, -1, 0): -2,
                   (2, 0, -1): 7,
                   (2, 0, 0): -15,
                   (2, 0, 1): -24,
                   (2, 1, 0): -20}},
 'xs': {'bits': {'b0': 1040596308, 'b1': 1037582655, 'b2': 1015904472},
        'cells': {(0, -1, 0): -6,
                  (0, 0, -1): -24,
                  (0, 0, 0): -21,
                  (0, 0, 1): 4,
                  (0, 1, 0): 8,
                  (1, -1, -1): 3,
                  (1, -1, 0): 2,
                  (1, -1, 1): -19,
                  (1, 0, -1): 1,
                  (1, 0, 0): 8,
                  (1, 0, 1): 4,
                  (1, 1, -1): 7,
                  (1, 1, 0): 4,
                  (1, 1, 1): -10,
                  (2, -1, 0): 6,
                  (2, 0, -1): -3,
                  (2, 0, 0): -15,
                  (2, 0, 1): -19,
                  (2, 1, 0): -5}},
 'xy': {'bits': {'b0': 3195786133, 'b1': 1049000183, 'b2': 1051573090},
        'cells': {(0, -1, 0): -8,
                  (0, 0, -1): 0,
                  (0, 0, 0): -10,
                  (0, 0, 1): -9,
                  (0, 1, 0): -15,
                  (1, -1, -1): -16,
                  (1, -1, 0): 0,
                  (1, -1, 1): -21,
                  (1, 0, -1): 5,
                  (1, 0, 0): 8,
                  (1, 0, 1): 7,
                  (1, 1, -1): -14,
                  (1, 1, 0): 6,
                  (1, 1, 1): -35,
                  (2, -1, 0): 3,
                  (2, 0, -1): -2,
                  (2, 0, 0): 5,
                  (2, 0, 1): -22,
                  (2, 1, 0): -20},
        'edge': 1090693803},
 'ys_gt': {'bits': {'b0': 1052231395, 'b1': 3199468648, 'b2': 3192537771},
           'cells': {(0, -1, 0): 7,
                     (0, 0, -1): -22,
                     (0, 0, 0): -2,
                     (0, 0, 1): -23,
                     (0, 1, 0): -9,
                     (1, -1, -1): -8,
                     (1, -1, 0): 1,
                     (1, -1, 1): 7,
                     (1, 0, -1): 7,
                     (1, 0, 0): 8,
                     (1, 0, 1): 4,
                     (1, 1, -1): -13,
                     (1, 1, 0): -12,
                     (1, 1, 1): -22,
                     (2, -1, 0): 5,
                     (2, 0, -1): -21,
                     (2, 0, 0): -3,
                     (2, 0, 1): -46,
                     (2, 1, 0): 6},
           'edge': 1092976309}}


def pivot(which, edge_thr):
    e = PIVOT[which]
    score = from_bits(e["edge"]) if "edge" in e else None
    if score is not None and score >= edge_thr:
        return Stencil("pivot_" + which, e["cells"], [(0, 0)], EDGE_HIGH, bits_={"edge": e["edge"]})
    return Stencil("pivot_" + which, e["cells"], [(0, 0)], KEPT, bits_=e["bits"])


def searched(name):
    e = SEARCHED[name]
    ar, ac = e.get("anchor", (0, 0))   # the claimed candidate's first centre among the cells
    sh = lambda q: (q[0] - ar, q[1] - ac)
    st = Stencil(name, {(p,) + sh((dr, dc)): v for (p, dr, dc), v in e["cells"].items()}, [sh(q) for q in e["path"]], e["exit"], bits_=e.get("bits"),
                 others=[(dl,) + sh((dr, dc)) + ([sh(q) for q in pth], ex) for dl, dr, dc, pth, ex in e.get("others", ())],
                 tuned={(p,) + sh((dr, dc)): u for (p, dr, dc), u in TUNED.get(name, {}).items()})
    if "bits_at" in e:   # b[k] of the iteration at `centre`, which the trace shows only when it is the last
        centre, k, u = e["bits_at"]
        st.bits_at = (sh(centre), k, u)
    return st


# L[level+1] around the final centre (dr, dc relative to the FIRST centre): Lxx = p[-1] - 2 p[0] + p[1] (pyramid.cpp:29)
def l_cells(at, kind, elsewhere=None):
    r, c = at
    row = {"neg": (F(0), F(3), F(0)), "pos": (F(3), F(0), F(0)), "zero": (F(1), F(1), F(1)), "negzero": (F(-0.0), F(0.0), F(-0.0))}[kind]
    out = {(r, c - 1): row[0], (r, c): row[1], (r, c + 1): row[2]}
    if elsewhere is not None:
        # the other type at the first centre, one column left of the final one: its p[0] and p[1] are cells of the final centre's row,
        # its p[-1] decides: Lxx = p[-1] - 2 p[0] + p[1] = 5 + 3 > 0 under a final "neg", -5 - {2 - 1, 6, 0} < 0 under the others
        er, ec = elsewhere
        assert (er, ec + 1) == (r, c)
        out[(er, ec - 1)] = F(5) if kind == "neg" else F(-5)
    return out


def l_type(L, level, r, c):
    """getHessianPointType (pyramid.cpp:24-37) of a positive response at (r, c): Lxx < 0 ? 0 : 1"""
    p = L[level + 1][r]
    return 0 if F(F(p[c - 1] - F(F(2) * p[c])) + p[c + 1]) < 0 else 1


L_TYPE = {"neg": 0, "pos": 1, "zero": 1, "negzero": 1}   # getHessianPointType: Lxx < 0 ? 0 : 1 for a positive response


# ----------------------------------------------------------------------------------------------------------------------
# Sites and planes
# ----------------------------------------------------------------------------------------------------------------------
class Site:
    def __init__(self, kind, stencil, level, r0, c0, group=None):
        self.kind = kind; self.stencil = stencil; self.level = level; self.r0 = r0; self.c0 = c0
        self.group = group   # sites of one group may be closer to each other than the spacing rule allows

    def __repr__(self):
        return "%s/%s@L%d(%d,%d)" % (self.kind, self.stencil.name, self.level, self.r0, self.c0)

    def walk(self, path, exit_, rows, cols, r0, c0):
        """(iters, final (r, c), exit, path) of a path on a rows x cols plane: it stops where a border test (pyramid.cpp:160-163,
        in that order) fails"""
        pth = [(r0 + dr, c0 + dc) for dr, dc in path]
        for k in range(len(pth) - 1):
            (r, c), (nr, nc) = pth[k], pth[k + 1]
            ex = None
            if nc > c and not c < cols - 3: ex = OUT_RIGHT
            elif nr > r and not r < rows - 3: ex = OUT_DOWN
            elif nc < c and not c > 3: ex = OUT_LEFT
            elif nr < r and not r > 3: ex = OUT_UP
            if ex is not None:
                return k + 1, (r, c), ex, pth[:k + 1]
        return len(pth), pth[-1], exit_, pth

    def claims(self, rows, cols):
        """-> [(level, r0, c0, claim)]: claim None = no candidate there; () = a candidate, nothing else claimed;
        else (iters, final (r, c), exit, path)"""
        st = self.stencil
        out = []
        if not st.path:
            out.append((self.level, self.r0, self.c0, None))
        elif st.exit is None:
            out.append((self.level, self.r0, self.c0, ()))
        else:
            out.append((self.level, self.r0, self.c0, self.walk(st.path, st.exit, rows, cols, self.r0, self.c0)))
        for dl, dr, dc, pth, ex in st.others:
            out.append((self.level + dl, self.r0 + dr, self.c0 + dc, () if pth is None else self.walk([(a - dr, b - dc) for a, b in pth], ex, rows, cols, self.r0 + dr, self.c0 + dc)))
        return out


def build(rows, cols, sites, seed):
    """-> L[5, rows, cols], R[5, rows, cols] float32 with the sites written and R's frame filled with seeded garbage"""
    L = np.zeros((5, rows, cols), F); R = np.zeros((5, rows, cols), F)
    boxes = []
    for s in sites:
        st = s.stencil
        for (p, dr, dc), v in st.cells.items():
            r, c = s.r0 + dr, s.c0 + dc
            assert 1 <= r <= rows - 2 and 1 <= c <= cols - 2 and s.level + p <= 4, (s, p, r, c)
            R[s.level + p, r, c] = v
        for (dr, dc), v in st.lcells.items():
            L[s.level + 1, s.r0 + dr, s.c0 + dc] = v
        r_lo, r_hi, c_lo, c_hi = st.box()
        boxes.append((s.r0 + r_lo, s.r0 + r_hi, s.c0 + c_lo, s.c0 + c_hi))
    for i in range(len(boxes)):
        for j in range(i):
            a, b = boxes[i], boxes[j]
            if sites[i].group is not None and sites[i].group == sites[j].group:
                continue
            gap_r = max(a[0] - b[1], b[0] - a[1]); gap_c = max(a[2] - b[3], b[2] - a[3])
            assert gap_r >= 3 or gap_c >= 3, ("sites too close", sites[i], sites[j])
    garbage(R, seed)
    return L, R


def garbage(R, seed):
    """large finite values of both signs on the frame of every plane of R"""
    rng = np.random.RandomState(seed)
    for p in range(R.shape[0]):
        for sl in ((0, slice(None)), (-1, slice(None)), (slice(None), 0), (slice(None), -1)):
            n = R[p][sl].shape[0]
            R[p][sl] = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(3, 37, n)).astype(F)
    return R


def comb(rows, cols, row, seed):
    """every second scanned column of `row` is a maximum of R[1] and of R[2] (equal: candidates at levels 0 and 1, the lower
    level kept, the upper TAKEN): 62 candidates per ballot group of a full strip, so the second group of a level does not fit what
    is left of the wavefront's block of 64 and forces a refill with holes in the middle of the row.  -> Sites (two_levels)."""
    rng = np.random.RandomState(seed)
    out = []
    for c in range(BORDER, cols - BORDER, 2):
        out.append(Site("comb", two_levels(F(64 + 8 * rng.randint(0, 16))), 0, row, c, group="comb"))
    return out


def local_system(R, level, r, c):
    """A[9], rhs[3] of localizeKeypoint's linear system at centre (r, c) of `level` (pyramid.cpp:132-150), the same float32
    operations in the same order.  For the claims about iterations the trace does not show, and about the pivot ties."""
    low, cur, high = R[level], R[level + 1], R[level + 2]
    two = F(2.0); q = F(0.25); h = F(0.5)
    dxx = F(F(cur[r, c - 1] - F(two * cur[r, c])) + cur[r, c + 1])
    dyy = F(F(cur[r - 1, c] - F(two * cur[r, c])) + cur[r + 1, c])
    dss = F(F(low[r, c] - F(two * cur[r, c])) + high[r, c])
    dxy = F(q * F(F(F(cur[r + 1, c + 1] - cur[r + 1, c - 1]) - cur[r - 1, c + 1]) + cur[r - 1, c - 1]))
    dxs = F(q * F(F(F(high[r, c + 1] - high[r, c - 1]) - low[r, c + 1]) + low[r, c - 1]))
    dys = F(q * F(F(F(high[r + 1, c] - high[r - 1, c]) - low[r + 1, c]) + low[r - 1, c]))
    dx = F(h * F(cur[r, c + 1] - cur[r, c - 1]))
    dy = F(h * F(cur[r + 1, c] - cur[r - 1, c]))
    ds = F(h * F(high[r, c] - low[r, c]))
    return np.array([dxx, dxy, dxs, dxy, dyy, dys, dxs, dys, dss], F), np.array([-dx, -dy, -ds], F)


def edge_score(st):
    """the first iteration's edgeScore of a stencil's first centre (pyramid.cpp:144), float32 as the chain computes it"""
    R = np.zeros((3, 5, 5), F)
    for (p, dr, dc), v in st.cells.items():
        if abs(dr) <= 2 and abs(dc) <= 2 and p < 3:
            R[p, 2 + dr, 2 + dc] = v
    A, _ = local_system(R, 0, 2, 2)
    dxx, dxy, dyy = A[0], A[1], A[4]
    with np.errstate(all="ignore"):
        return F(F(F(dxx + dyy) * F(dxx + dyy)) / F(F(dxx * dyy) - F(dxy * dxy)))


def cross_near(side):
    """-> the cross whose edgeScore is the float32 adjacent to 6.25 on one side, and that score"""
    st = cross(16.0, 64.0, *CROSS_NEAR[side], name="cross_" + side)
    return st, edge_score(st)


# ----------------------------------------------------------------------------------------------------------------------
# The catalogue: every stencil kind once (its claim depends on the parameter set only through the thresholds)
# ----------------------------------------------------------------------------------------------------------------------
def catalogue(pset):
    """-> [(kind, stencil, level)]"""
    pos, final, edge_thr = thresholds(pset)
    out = []
    lv = [0]

    def add(kind, st, level=None):
        if level is None:
            level = lv[0] % 3; lv[0] += 1
        out.append((kind, st, level))

    # thresholds: val == the pixel.  `val > positiveThreshold` (pyramid.cpp:213) and `fabsf(val) < finalThreshold` (:166)
    for neg in (False, True):
        for name, v, path, ex in (("at_pos", pos, [], None), ("above_pos", step(pos, 1), [(0, 0)], WEAK),
                                  ("at_final", final, [(0, 0)], KEPT), ("below_final", step(final, -1), [(0, 0)], WEAK)):
            st = peak(v, "thr_" + name)
            st.path = path; st.exit = ex
            add("threshold", st.negated() if neg else st)
    # edge score: 6.25 is the threshold of edgeEigenValueRatio = 4 exactly (`edgeScore >= threshold`, pyramid.cpp:145)
    st = cross(16.0, 64.0); st.bits["edge"] = bits(F(6.25)); st.exit = EDGE_HIGH if F(6.25) >= edge_thr else KEPT
    add("edge", st)
    for side in ("below", "above"):
        st, e = cross_near(side)
        st.bits["edge"] = bits(e); st.exit = EDGE_HIGH if e >= edge_thr else KEPT
        add("edge", st)
    add("edge", saddle(64.0)); add("edge", plateau(64.0)); add("edge", plateau_min(64.0))
    # ties
    for name, offs in (("h2", [(0, 0), (0, 1)]), ("h3", [(0, 0), (0, 1), (0, 2)]), ("v2", [(0, 0), (1, 0)]), ("v3", [(0, 0), (1, 0), (2, 0)]),
                       ("d2", [(0, 0), (1, 1)]), ("d3", [(0, 0), (1, 1), (2, 2)]), ("a2", [(0, 0), (1, -1)])):
        add("ties", ties(offs, 96.0, "ties_" + name, [KEPT, EDGE_NEG, KEPT] if name in ("h3", "v3") else None))
    add("ties", two_levels(80.0), 0); add("ties", two_levels(80.0), 1)
    # pivot ties of the solve
    for which in ("xy", "xs", "ys_gt", "a47"):
        add("pivot", pivot(which, edge_thr), 0)
    # moves: one in each direction, a diagonal one, chains, the fifth iteration
    c1 = searched("chain1")
    for st in (c1, c1.mirrored(), c1.transposed(), c1.transposed().mirrored_rows()):
        add("move", st)
    add("move", searched("diag"), 0)
    for n in ("chain2", "chain3", "chain4", "still5"):
        add("move", searched(n)); add("move", searched(n).transposed())
    # the double 0.6 from both sides at the second iteration, and -0.6 by the mirror image
    for n in ("b0_06_below", "b0_06_above", "b1_06_below", "b1_06_above"):
        st = searched(n)
        lvl = 0 if n.endswith("above") else None   # (tuned after the search: on a higher level a candidate of the level below takes its cell)
        add("shift06", st, lvl); add("shift06", st.mirrored() if n.startswith("b0") else st.mirrored_rows(), lvl)
    # |b[k]| == 1.5 is kept, a step above is dropped (`fabsf(b) > 1.5`, pyramid.cpp:166)
    add("shift15", searched("b0_15")); add("shift15", searched("b0_15").mirrored()); add("shift15", searched("b0_15_above"))
    add("shift15", searched("b0_15").transposed()); add("shift15", searched("b1_15_above"))
    add("shift15", searched("b2_15")); add("shift15", searched("b2_15_above"))
    # type (getHessianPointType, pyramid.cpp:24-37): Lxx at the FINAL centre; a moved site has the other type at its first centre
    for kind in ("neg", "pos", "zero", "negzero"):
        st = peak(F(64.0))
        st = st.with_l("L" + kind, l_cells((0, 0), kind))
        st.type = L_TYPE[kind]
        add("type", st)
        st = c1.with_l("L" + kind, l_cells(c1.path[-1], kind, elsewhere=(0, 0)))
        st.type = L_TYPE[kind]
        add("type", st, 0)
    # collisions (the octaveMap rule, pyramid.cpp:166-170: the first in scan order - level, r0, c0 - keeps the cell)
    for n in ("pair", "lowerwins", "threeway", "loserneighbour"):
        add("collision", searched(n), 0)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# Layout: where the sites go
# ----------------------------------------------------------------------------------------------------------------------
class Layout:
    def __init__(self, rows, cols):
        self.rows = rows; self.cols = cols; self.sites = []
        self.boxes = np.zeros((0, 4), np.int64)
        self.cursor = (BORDER + 1, BORDER + 1)

    def fits(self, st, r0, c0):
        if not (BORDER <= r0 < self.rows - BORDER and BORDER <= c0 < self.cols - BORDER):
            return False
        r_lo, r_hi, c_lo, c_hi = st.box()
        a = (r0 + r_lo, r0 + r_hi, c0 + c_lo, c0 + c_hi)
        if a[0] < 1 or a[1] > self.rows - 2 or a[2] < 1 or a[3] > self.cols - 2:
            return False
        b = self.boxes
        gap_r = np.maximum(a[0] - b[:, 1], b[:, 0] - a[1]); gap_c = np.maximum(a[2] - b[:, 3], b[:, 2] - a[3])
        return bool(np.all((gap_r >= 3) | (gap_c >= 3)))

    def put(self, kind, st, level, r0, c0, group=None, check=True):
        assert not check or self.fits(st, r0, c0), (kind, st.name, r0, c0)
        r_lo, r_hi, c_lo, c_hi = st.box()
        self.boxes = np.vstack([self.boxes, [[r0 + r_lo, r0 + r_hi, c0 + c_lo, c0 + c_hi]]])
        self.sites.append(Site(kind, st, level, r0, c0, group))

    def at_col(self, kind, st, level, c0):
        for r0 in range(BORDER, self.rows - BORDER):
            if self.fits(st, r0, c0):
                return self.put(kind, st, level, r0, c0)
        raise AssertionError("no room for %s/%s at column %d of %d x %d" % (kind, st.name, c0, self.rows, self.cols))

    def at_row(self, kind, st, level, r0):
        for c0 in range(16, self.cols - 16):
            if self.fits(st, r0, c0):
                return self.put(kind, st, level, r0, c0)
        raise AssertionError("no room for %s/%s at row %d of %d x %d" % (kind, st.name, r0, self.rows, self.cols))

    def anywhere(self, kind, st, level):
        r, c = self.cursor
        while r < self.rows - BORDER - 1:
            while c < self.cols - BORDER - 1:
                if self.fits(st, r, c):
                    self.cursor = (r, c)
                    return self.put(kind, st, level, r, c)
                c += 1
            r += 1; c = BORDER + 1
        raise AssertionError("no room for %s/%s on %d x %d" % (kind, st.name, self.rows, self.cols))


def special_cols(cols, thorough=True):
    """first and last scanned columns, each column of a lane (c mod 4), the lane seam 243 | 244 and the strip seams 247 | 248, 495 | 496"""
    c = {5, 6, 7, 8, cols - 6, cols - 7, cols - 8, cols - 9, 243, 244, 247, 248, 495, 496}
    if not thorough:   # (the small shapes: the seams and the two ends)
        c = {5, cols - 6, cols - 7, 243, 244, 247, 248}
    return sorted(x for x in c if BORDER <= x < cols - BORDER)


def special_rows(rows):
    """first and last scanned rows and the rows on both sides of every band seam of bands 32, 64 and 128"""
    r = {5, rows - 6}
    for band in (32, 64, 128):
        for k in range(1, rows // band + 1):
            r |= {k * band - 1, k * band}
    return sorted(x for x in r if BORDER <= x < rows - BORDER)


def position_sites(rows, cols, thorough=True, lay=None):
    """the cheap kinds - the zero-gradient kept site and the one-move site - at every special position, and the border chains.
    thorough: both directions of the move at every position (else one, alternating)"""
    lay = lay or Layout(rows, cols)
    c1 = searched("chain1"); c2 = searched("chain2"); c3 = searched("chain3")
    right, left, down, up = c1, c1.mirrored(), c1.transposed(), c1.transposed().mirrored_rows()
    n = [0]

    def level():
        n[0] += 1
        return n[0] % 3

    if thorough:
        # Chains that walk out through a border test, or come to rest next to it and are kept.  The tests are not mirror images
        # (pyramid.cpp:160-163: `c < cols - 3` lets a centre reach cols - 3, `c > 3` stops it at 3):
        #   left / up     5 -> 4 -> 3, then asks for 2: out; 5 -> 4 -> 3 and rests: kept
        #   right / down  n-6 -> n-5 -> n-4 -> n-3, then asks for n-2: out (its last cells, on the frame, are cut: never read);
        #                 n-6 -> .. -> n-3 and rests: kept; n-6 -> n-5 -> n-4 and rests: kept
        c4 = searched("chain4").cut(4)
        for st in (c3.mirrored(), c2.mirrored()):
            lay.at_col("border", st, level(), 5)
        for st in (c4, c3, c2):
            lay.at_col("border", st, level(), cols - 6)
        for st in (c3.transposed().mirrored_rows(), c2.transposed().mirrored_rows()):
            lay.at_row("border", st, level(), 5)
        for st in (c4.transposed(), c3.transposed(), c2.transposed()):
            lay.at_row("border", st, level(), rows - 6)
    for i, c in enumerate(special_cols(cols, thorough)):
        moves = [m for m in ((right, left) if thorough else ((right, left) if i % 2 else (left, right))[:1]) if lay_ok(m, c, cols, 2)]
        for st in [peak(F(72.0 + 8 * (i % 5)))] + moves:
            lay.at_col("position", st, level(), c)
    for i, r in enumerate(special_rows(rows)):
        moves = [m for m in ((down, up) if thorough else ((down, up) if i % 2 else (up, down))[:1]) if lay_ok(m, r, rows, 1)]
        for st in [peak(F(-72.0 - 8 * (i % 5)))] + moves:
            lay.at_row("position", st, level(), r)
    return lay.sites


def lay_ok(st, at, n, axis):
    """the stencil's cells stay inside the frame along one axis (axis 1: rows, 2: columns) when its first centre is at `at`"""
    b = st.box()
    lo, hi = (b[0], b[1]) if axis == 1 else (b[2], b[3])
    return at + lo >= 1 and at + hi <= n - 2


def catalogue_sites(rows, cols, pset, comb_row=None, seed=7, lay=None):
    """every stencil kind once, and the comb when a row is given"""
    lay = lay or Layout(rows, cols)
    if comb_row is not None:
        for s in comb(rows, cols, comb_row, seed):
            lay.put(s.kind, s.stencil, s.level, s.r0, s.c0, group="comb", check=False)
    for kind, st, level in catalogue(pset):
        lay.anywhere(kind, st, level)
    return lay.sites


def tiny_sites():
    """13 x 13, the smallest plane that is an octave: nine scanned pixels, four of them taken"""
    return [Site("position", peak(F(72.0)), 0, 5, 5, "tiny"), Site("position", peak(F(-88.0)), 1, 5, 7, "tiny"),
            Site("position", peak(F(96.0)), 2, 7, 5, "tiny"), Site("position", two_levels(F(80.0)), 0, 7, 7, "tiny")]


# ----------------------------------------------------------------------------------------------------------------------
# Scenes: name -> (rows, cols, sites)
# ----------------------------------------------------------------------------------------------------------------------
SMALL_SHAPES = [(r, c) for r in (37, 38) for c in (253, 254, 255, 256)]
SCENES = ["positions70", "catalogue70", "catalogue70b", "tiny", "all262"] + ["small%dx%d" % rc for rc in SMALL_SHAPES]


def scene(name, pset):
    """-> rows, cols, sites.
    positions70    70 x 510 (three strips; with band 32 three bands, the last with the single scanned row 64): the cheap kinds at every position
    catalogue70    70 x 510: every stencil kind and the comb;  catalogue70b: the same with other comb heights
    tiny           13 x 13
    small37x253 .. rows 37 (no scanned row in the second band) and 38 (one), the last scanned column 247 .. 250: a second strip with 0 .. 3
                   scanned columns, every cols mod 4
    all262         262 x 510: positions, catalogue and comb on one plane (run with bands 32, 64 and 128: three, two and one seam rows apart)"""
    if name == "positions70":
        return 70, 510, position_sites(70, 510)
    if name in ("catalogue70", "catalogue70b"):
        return 70, 510, catalogue_sites(70, 510, pset, comb_row=62, seed=7 if name == "catalogue70" else 8)
    if name == "tiny":
        return 13, 13, tiny_sites()
    if name == "all262":
        lay = Layout(262, 510)
        catalogue_sites(262, 510, pset, comb_row=110, seed=9, lay=lay)
        position_sites(262, 510, lay=lay)
        return 262, 510, lay.sites
    if name.startswith("small"):
        r, c = (int(x) for x in name[5:].split("x"))
        return r, c, position_sites(r, c, thorough=False)
    raise KeyError(name)


def planes(name, pset, garbage_seed=1):
    rows, cols, sites = scene(name, pset)
    L, R = build(rows, cols, sites, garbage_seed)
    return L, R, sites


def solve3x3(A, b, flip=None):
    """solveLinear3x3 (helpers.cpp:46-88) in float32, operation for operation -> b.  flip names ONE comparison that is decided the
    other way at equality: "first" (`tmp > vp` as >=), "second" (`fabsf(A[6]) > vp` as >=), "third" (`fabsf(A[4]) < fabsf(A[7])` as
    <=).  With flip=None it is the reference's solve (the CPU tests hold it against the oracle's, bit for bit); with a flip it is what
    an implementation would compute that took the other pivot at a tie - the pivot sites show that the result then differs."""
    A = [F(x) for x in A]; b = [F(x) for x in b]
    gt = lambda x, y, key: (x >= y) if flip == key else (x > y)
    i = 0
    vp = abs(A[0]); tmp = abs(A[3])
    if gt(tmp, vp, "first"):
        i = 1; vp = tmp
    if gt(abs(A[6]), vp, "second"):
        i = 2
    if i != 0:
        for k in range(3):
            A[3 * i + k], A[k] = A[k], A[3 * i + k]
        b[i], b[0] = b[0], b[i]
    with np.errstate(all="ignore"):
        vp = F(A[3] / A[0]); A[4] = F(A[4] - F(vp * A[1])); A[5] = F(A[5] - F(vp * A[2])); b[1] = F(b[1] - F(vp * b[0]))
        vp = F(A[6] / A[0]); A[7] = F(A[7] - F(vp * A[1])); A[8] = F(A[8] - F(vp * A[2])); b[2] = F(b[2] - F(vp * b[0]))
        if gt(abs(A[7]), abs(A[4]), "third"):
            A[7], A[4] = A[4], A[7]; A[8], A[5] = A[5], A[8]; b[2], b[1] = b[1], b[2]
        vp = F(A[7] / A[4])
        A[8] = F(A[8] - F(vp * A[5]))
        b[2] = F(b[2] - F(vp * b[1]))
        b[2] = F(b[2] / A[8])
        b[1] = F(F(b[1] - F(A[5] * b[2])) / A[4])
        b[0] = F(F(F(b[0] - F(A[2] * b[2])) - F(A[1] * b[1])) / A[0])
    return np.array(b, F)
