"""Shapes and grids shared by test_solid_host.py and test_gpu_solid.py: closed meshes from the geometry primitives through
mesh.Mesh (which winds every face outward), with a grid over their bounding box."""
import numpy as np


def _mesh(v, f):
    from nanokappa_amd.mesh import Mesh
    return Mesh(v, f)


def turned_castle():
    """The castle with its axis along x: five sections of length 10, so a grid of 5 cells along x has its planes ON the flat
    annular lids (faces lying in grid planes perpendicular to x: the double-count case of the ownership rule)."""
    from nanokappa_amd import geometry as G
    v, f = G.castle_primitive([10, 10, 8, 5, 8, 5, 1])
    return v[:, [2, 0, 1]], f


def shape(name):
    from nanokappa_amd import geometry as G
    if name == 'box':
        return _mesh(*G.box_primitive([30, 20, 10]))
    if name == 'cyl12':
        return _mesh(*G.cylinder_primitive([30, 10, 12]))
    if name == 'cyl7':
        return _mesh(*G.cylinder_primitive([30, 10, 7]))
    if name == 'corrugated':
        return _mesh(*G.corrugated_primitive([10, 8, 5, 9, 4]))
    if name == 'star':
        return _mesh(*G.star_primitive([10, 10, 4, 5]))
    if name == 'castle':
        return _mesh(*G.castle_primitive([10, 6, 8, 5, 8, 3, 1]))
    if name == 'turned_castle':
        return _mesh(*turned_castle())
    raise KeyError(name)


# (shape, cells): the cases of the host tests
CASES = [('box', (3, 2, 2)), ('cyl12', (4, 4, 3)), ('cyl7', (5, 3, 2)), ('corrugated', (3, 4, 5)), ('star', (5, 5, 2)),
         ('castle', (4, 4, 6)), ('turned_castle', (5, 3, 3)), ('turned_castle', (4, 3, 3))]

_MESHES = {}


def case(name, n, pad=0):
    """(mesh, lo, h, n) of a shape on n cells over its bounding box; pad: that many more cells of the same size on every side."""
    from nanokappa_amd import field as FD
    if name not in _MESHES:
        _MESHES[name] = shape(name)
    m = _MESHES[name]
    lo, h, n = FD.grid_from_bounds(np.array([m.vertices.min(axis=0), m.vertices.max(axis=0)]), n)
    if pad:
        lo, n = lo - pad * h, tuple(k + 2 * pad for k in n)
    return m, lo, h, n
