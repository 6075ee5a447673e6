"""Kinetic maps on the CPU: the map tally of the kinetic flights (DESIGN.md "Kinetic maps") -- a segment's four words also go to the
line of (source, cell of the segment's point x_p) on the field's grid, the cell by nanokappa_amd.field.cell_index.  The rule, tally
included, stands once, in kinetic_cases.restate(grids=...); restate_map here names its results.  What the GPU tests hold
nk_kinetic_flights_map against, the grids they share and the per-cell isothermal check.  Test infrastructure: nothing under
nanokappa_amd/ knows of it."""
import math

import numpy as np

import kinetic_cases as K
import free_path_cases as FC
from free_path_cases import cached
from kinetic_cases import MAX_EVENTS

ROW_CLAMPED = 25              # NK_KIN_ROW_CLAMPED


def restate_map(grid, g, sv, group_vel, tau, c, n, seed=0, max_events=MAX_EVENTS, rough=None, J=None, fused=True, start_point=False, more=(),
                cosine=True, trace=None):
    """kinetic_cases.restate(g, sv, group_vel, tau, c, n, ...) with the map tally on grid = (lo, h, n_cells): returns its dict (rows
    with word 25 = clamped) and map [F, nx, ny, nz, 4] int64, dwell_map, flux_map, clamped [F].  start_point=True bins the segment's
    START point x instead of x_p: the WRONG rule, for the sensitivity check of the isothermal test.  more: further (grid,
    start_point) pairs tallied over the same flights -> `map_more`, a list of (map, clamped)."""
    r = K.restate(g, sv, group_vel, tau, c, n, seed=seed, max_events=max_events, rough=rough, J=J, fused=fused, cosine=cosine, trace=trace,
                  grids=((grid, start_point),) + tuple(more))
    maps = r.pop('grids')
    mp, cl = maps[0]
    r['rows'][:, ROW_CLAMPED] = cl
    return dict(r, map=mp, dwell_map=mp[..., 0] / 2.0 ** r['report']['k_t'], flux_map=mp[..., 1:4] / 2.0 ** r['report']['k_x'],
                clamped=cl.copy(), map_more=maps[1:])


# ------------------------------------------------------------------------------------------- grids and cases
def transport_axis(ct):
    """The axis of the first source's normal: x on the boxes, z on the wire."""
    return int(np.argmax(np.abs(K.source_geometry(ct)[2][0])))


def grid_for(ct, n_cells):
    """(lo, h, n_cells) over the mesh's bounds (field.grid_from_bounds)."""
    from nanokappa_amd import field as FD
    return FD.grid_from_bounds(np.asarray(ct['mesh']['bounds'], dtype=np.float64).reshape(2, 3), n_cells)


def middle_half(ct, n_cells):
    """A caller's grid that covers only the middle half of the bounds along x (all of y and z): segment points in the outer
    quarters are clamped into its edge cells."""
    lo, h, n = grid_for(ct, n_cells)
    b = np.asarray(ct['mesh']['bounds'], dtype=np.float64).reshape(2, 3)
    lo, h = lo.copy(), h.copy()
    lo[0] = b[0, 0] + 0.25 * (b[1, 0] - b[0, 0])
    h[0] = 0.5 * (b[1, 0] - b[0, 0]) / n[0]
    return lo, h, n


def parity_cells(name):
    """The cell counts a PARITY case is flown with: (5, 3, 2), (1, 1, 1) and 7 cells along the transport axis -- cell sizes that
    are no binary fractions, odd counts."""
    seven = [1, 1, 1]
    seven[transport_axis(K.case(K.PARITY[name]['case']))] = 7
    return ((5, 3, 2), (1, 1, 1), tuple(seven))


def run_case(name, n, seed, scale, grids, max_events=MAX_EVENTS):
    """The map restatement on a named case for the grids ((lo, h, n_cells, start_point), ...) given as hashable tuples, all over the
    same flights (cached): the dict of the first, with `map_more` for the others."""
    def make():
        ct = K.case(name)
        gs = [((np.array(lo), np.array(h), nc), sp) for lo, h, nc, sp in grids]
        return restate_map(gs[0][0], ct['mesh'], K.subvols(ct), FC.group_vel(ct), K.lifetimes(ct, scale), K.heat_capacity(ct), n, seed=seed,
                           max_events=max_events, rough=ct['rough'], J=ct['J'], start_point=gs[0][1], more=tuple(gs[1:]))
    return cached(('kin_map_run', name, n, seed, scale, tuple(grids), max_events), make)


def key_of(grid, start_point=False):
    lo, h, nc = grid
    return tuple(float(a) for a in lo), tuple(float(a) for a in h), tuple(int(a) for a in nc), bool(start_point)


def map_of(run, j):
    """(map, clamped) of the j-th grid of a run_case() result."""
    return (run['map'], run['clamped']) if j == 0 else run['map_more'][j - 1]


def parity_run(name):
    """The restatement of a PARITY case on parity_cells(name) over the bounds and, last, on (4, 2, 2) over the middle half."""
    p = K.PARITY[name]
    ct = K.case(p['case'])
    grids = [key_of(grid_for(ct, nc)) for nc in parity_cells(name)] + [key_of(middle_half(ct, (4, 2, 2)))]
    return run_case(p['case'], K.PARITY_N, p['seed'], p['scale'], tuple(grids))


# The per-cell isothermal identity: every source 1 K above the reference gives dT = 1 and q = 0 in every cell.  K.STAT's two cases
# with their seeds and N, and the wire with the exact solid volume of every cell; N, the seeds and the grids were chosen on the
# CPU so that the restatement passes (test_kinetic_map_host.py states the figures); the Student-t remark at K.STAT applies.
STAT = {
    'ttp_16': dict(case='ttp', scale=1.0 / 16.0, n=K.STAT['ttp_16']['n'], seeds=K.STAT['ttp_16']['seeds'], cells=(4, 2, 2), volume='cell'),
    'box3': dict(case='box3', scale=1.0, n=K.STAT['box3']['n'], seeds=K.STAT['box3']['seeds'], cells=(3, 2, 2), volume='cell'),
    'wire72': dict(case='wire72', scale=1.0, n=2048, seeds=tuple(range(300, 308)), cells=(4, 4, 2), volume='solid'),
}
MAX_DEVIATION = 5.0           # standard errors, from the 8 calls
MIN_SOLID = 0.05              # wire: cells with a smaller solid fraction may be left out ...
MAX_LEFT_OUT = 0.25           # ... but never more than this share of the cells that hold solid
MIN_POWER = 10.0              # the start-point rule must miss by more than this many standard errors


def stat_grid(name):
    p = STAT[name]
    return grid_for(K.case(p['case']), p['cells'])


def stat_volume(name, solid_volume=None):
    """(V [nx, ny, nz], keep mask) of a statistical case: the cell volume, or the solid volume of every cell (field.solid_volume on
    the CPU unless given) with the cells under MIN_SOLID left out."""
    from nanokappa_amd import field as FD
    p = STAT[name]
    lo, h, nc = stat_grid(name)
    cell = float(np.prod(h))
    if p['volume'] == 'cell':
        return np.full(nc, cell), np.ones(nc, dtype=bool)
    if solid_volume is None:
        g = K.case(p['case'])['mesh']
        solid_volume = cached(('kin_map_solid', name), lambda: FD.solid_volume(g['vertices'], g['faces'], lo, h, nc))
    V = np.asarray(solid_volume, dtype=np.float64).reshape(nc)
    keep = V / cell >= MIN_SOLID
    assert (~keep & (V > 0)).sum() <= MAX_LEFT_OUT * (V > 0).sum()
    return V, keep


def stat_runs(name):
    """The map restatement's 8 calls of a statistical case, each with the grid under the right and under the start-point rule."""
    p = STAT[name]
    g = stat_grid(name)
    return [run_case(p['case'], p['n'], s, p['scale'], (key_of(g), key_of(g, True))) for s in p['seeds']]


def isothermal_cells(res, ct, tau, V):
    """(dT [nx, ny, nz] K, q [nx, ny, nz, 3] W/m^2) of one map result with every source 1 K above the reference, through
    kinetic_map.cell_profile (kinetic.profile on the cells): 1 and 0 in the exact solution."""
    from nanokappa_amd import kinetic as KN
    from nanokappa_amd import kinetic_map as KM
    c = K.heat_capacity(ct)
    lv = KN.live_modes(c, tau)
    src, area, n_in, _ = K.source_geometry(ct)
    g = KN.source_strength(area, n_in, c, FC.group_vel(ct), lv)
    dT, q = KM.cell_profile(res, g, np.ones(src.shape[0]), V, math.fsum(c[lv]))
    return dT.reshape(V.shape), q.reshape(V.shape + (3,))


def isothermal_deviation(results, ct, tau, V, keep):
    """(worst |mean dT - 1| / se, worst se of dT, worst |mean q| / se) over the kept cells, from the calls' dwell_map / flux_map."""
    dT, q = zip(*(isothermal_cells(r, ct, tau, V) for r in results))
    m, se = K.mean_se(np.array(dT)[:, keep])
    mq, sq = K.mean_se(np.array(q)[:, keep])
    return float(np.max(np.abs(m - 1.0) / se)), float(se.max()), float(np.max(np.abs(mq) / sq))


def as_result(n, dwell_map, flux_map):
    return dict(n=n, dwell_map=dwell_map, flux_map=flux_map)
