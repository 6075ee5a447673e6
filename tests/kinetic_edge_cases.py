"""Kinetic flights at their edges: the inputs on which a ray ends other than by absorption (lost after 64 refused trials, capped at
max_events), on which terms above their bounds are left out of the integer sums and counted, on which modes sit (v = 0), on which
a specular turn lands in a mode that does not live, with six and eight sources, with launch shapes that leave lanes idle, and with
more bins than the LDS holds.  Each case is built from a case of kinetic_cases.py with plain arrays tau and c; the CPU restatement
(kinetic_cases.restate, kinetic_group_cases.restate_grouped) and Engine.kinetic_flights take the same arrays.
test_kinetic_edges_host.py holds the restatement to the edge each case is built for, test_gpu_kinetic_edges.py the kernel to the
restatement.  Test infrastructure: nothing under nanokappa_amd/ knows of it.

Left out: a case of its own for `missed` (it needs a mesh with a hole) and the draw u = 0 of a free time (it cannot be forced
through Philox).  'dead_turn' meets `missed` all the same: the scattering after a turn into a dead mode happens on the wall, and
the rays it sends outwards find no facet."""
import contextlib

import numpy as np

import kinetic_cases as K
import kinetic_group_cases as KGC
import free_path_cases as FC
from free_path_cases import cached

# name -> what the builders below need.  Seeds are chosen on the CPU so that fused and unfused positions give the same event
# sequence on every ray (test_kinetic_edges_host.py asserts it).
CASES = {
    'all_lost': dict(base='ttp', n=256, seed=301),
    'some_lost': dict(base='ttp', n=128, seed=302, max_events=1024),
    'capped_1': dict(base='ttp', n=128, seed=303, max_events=1),
    'capped_2': dict(base='ttp', n=128, seed=303, max_events=2),
    'capped_5': dict(base='ttp', n=128, seed=303, max_events=5),
    'stationary': dict(base='ttp', n=128, seed=304),
    'dead_turn': dict(base='ttrrp_k', n=128, seed=305, max_events=4096),
    'leftout_segment': dict(base='ttrrp_k', n=128, seed=306, max_events=64),
    'leftout_ray': dict(base='ttp', n=256, seed=326),
    'six_sources': dict(base='ttp', n=64, seed=308),
    'eight_sources': dict(base='wire72', n=64, seed=309),
    'bins_do_not_fit': dict(base='box128', n=128, seed=310),
}
LEAVES_OUT = ('leftout_segment', 'leftout_ray')
THREE_WAYS = ('some_lost', 'capped_2', 'leftout_segment', 'six_sources')
GROUPED = ('dead_turn', 'leftout_segment', 'leftout_ray', 'capped_2', 'stationary', 'six_sources')
SHAPES = ((1, 0), (1, 1), (65, 64), (100, 7), (256, 1))          # (n, rays_per_wave) on the 'ttp_16' parity inputs
EIGHT_SOURCES = (0, 1, 2, 3, 4, 5, 6, 73)           # wire72's 'T' facets: both caps (0 and 73) and the first six side facets
# 'bins_do_not_fit': nk_set_subvolumes takes at most 512 subvolumes, and the tables every geometry kernel keeps in LDS (352 bytes per
# subvolume) leave the 64 KB of a kinetic launch well before that, so the bins are pushed out by the sources instead: a box of 128
# slices with all six facets 'T' needs 6 x 128 x 32 B = 24 KB of bins behind 48 KB of tables (with two sources they would fit)
BOX128_ARGS = ['--geometry', 'box', '--dimensions', '200', '200', '200', '--subvolumes', 'slice', '128', '0',
               '--bound_pos', 'relative', '0', '.5', '.5', '1', '.5', '.5', '--bound_cond', 'T', 'T', 'R',
               '--bound_values', '302', '298', '5']


def base_case(name):
    if name != 'box128':
        return K.case(name)

    def make():
        from edge_cases import COMMON_ARGS
        from util import case_from_args
        return case_from_args(BOX128_ARGS + COMMON_ARGS)
    return cached(('kin_edge_base', name), make)


def _with_bc(ct, bc):
    g = dict(ct['mesh'])
    g['bound_cond'] = np.array(bc)
    return dict(ct, mesh=g)


def partners(ct):
    """[M] lists: the modes a specular turn can put a ray of mode m into (spec_map on every rough facet that reflects m truly, and
    the degenerate branch free_path_cases.restate takes with r1 >= 0.5)."""
    r, J = ct['rough'], ct['J']
    sm, ts = np.asarray(r['spec_map'], dtype=np.int64), np.asarray(r['true_spec']).astype(bool)
    M = sm.shape[1]
    dj = r.get('degen_j2')
    out = []
    for m in range(M):
        p = set()
        for f in range(sm.shape[0]):
            o = int(sm[f, m])
            if ts[f, m] and 0 <= o < M:
                p.add(o)
                if dj is not None and -1 < int(dj[o]) < J:
                    p.add((o // J) * J + int(dj[o]))
        out.append(sorted(p))
    return out


def turning_set(ct, candidates):
    """(A, P): a greedy set A of the candidate modes, each with at least one specular partner, none of them in A; P their partners."""
    part = partners(ct)
    A, P = set(), set()
    for m in candidates:
        m = int(m)
        if m in P or not part[m] or any(p in A or p == m for p in part[m]):
            continue
        A.add(m)
        P.update(part[m])
    return np.array(sorted(A)), np.array(sorted(P))


def inputs(name):
    """dict of a case: ct (a case_tables-shaped dict: mesh, rough, J, ...), tau, c [M], n, seed, max_events (0: the default) and
    `tables`, None or the function that replaces nanokappa_amd.kinetic.tables for the case (cached; callers must not modify it)."""
    def make():
        from nanokappa_amd import kinetic as KN
        p = CASES[name]
        ct = base_case(p['base'])
        v = FC.group_vel(ct)
        sp = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        tau, c = K.lifetimes(ct), K.heat_capacity(ct)
        live = KN.live_modes(c, tau)
        tables, extra = None, {}
        if name == 'all_lost':                  # only modes that fly along the source facets: (v . n)+ = 0, every trial is refused
            c = np.where(live & (v[:, 0] == 0) & (sp > 0), c, 0.0)
        elif name == 'some_lost':               # ... nearly only: an accepted trial is rare
            c = np.where(v[:, 0] != 0, c * 1e-4, c)
        elif name.startswith('capped_'):
            tau = K.lifetimes(ct, 1.0 / 16.0)
        elif name == 'stationary':              # the modes that do not move scatter, and carry most of the scattering weight
            tau = K.lifetimes(ct, 1.0 / 16.0)
            still = sp == 0
            tau = np.where(still & ~(tau > 0), np.median(tau[live]), tau)
            c = np.where(still, 50.0 * c[live].max(), c)
            extra['still'] = np.nonzero(still)[0]
        elif name in ('dead_turn', 'leftout_segment'):
            ct = dict(ct, rough=dict(ct['rough'], specularity=np.ones_like(np.asarray(ct['rough']['specularity'], dtype=np.float64))))
            cand = np.nonzero(live & (sp > 0))[0]
            if name == 'leftout_segment':       # the slower half: their partners' casts take longer than the bounds allow
                cand = cand[sp[cand] <= np.median(sp[cand])]
            A, P = turning_set(ct, cand)
            keep = np.zeros(c.shape, dtype=bool)
            keep[A] = True
            c = np.where(keep, c, 0.0)
            tau = tau.copy()
            if name == 'dead_turn':
                tau[P] = 0.0
            else:
                tau[A], tau[P] = 0.125, 1e30
            extra.update(A=A, P=P)
        elif name == 'leftout_ray':             # every scattering would go to the slowest moving live mode s, whose bounds are
            mv = np.nonzero(live & (sp > 0))[0]         # tiny -- but no ray scatters: the bounds fit no flight
            s = int(mv[np.argmin(sp[mv])])
            tau = np.where(live, 1e30, tau)
            tau[s] = 2.0 ** -12
            orig = KN.tables

            def tables(c_, tau_, vg_):
                cs, cf = orig(c_, tau_, vg_)
                cs = np.zeros_like(cs)
                cs[s:] = 1.0
                return cs, cf
            extra['s'] = s
        elif name in ('six_sources', 'bins_do_not_fit'):
            ct = _with_bc(ct, ['T'] * 6)
            tau = K.lifetimes(ct, 1.0 / 4.0)
        elif name == 'eight_sources':
            bc = ['R'] * len(ct['mesh']['bound_cond'])
            for f in EIGHT_SOURCES:
                bc[f] = 'T'
            ct = _with_bc(ct, bc)
        return dict(extra, name=name, ct=ct, tau=tau, c=c, n=p['n'], seed=p['seed'], max_events=p.get('max_events', 0), tables=tables)
    return cached(('kin_edge_inputs', name), make)


@contextlib.contextmanager
def tables_of(inp):
    """nanokappa_amd.kinetic.tables replaced by the case's for the block (both the engine and the restatement call it by that name)."""
    from nanokappa_amd import kinetic as KN
    if inp['tables'] is None:
        yield
        return
    orig = KN.tables
    KN.tables = inp['tables']
    try:
        yield
    finally:
        KN.tables = orig


def group_table(M):
    """The edge cases' table: the modes split by index into three groups, every tenth mode sent to the rest column (-1)."""
    t = (np.arange(M, dtype=np.int64) * 3) // M
    t[::10] = -1
    return t.astype(np.int32)


def partner_table(inp):
    """'leftout_segment' with one group: the partner modes (never drawn by cdf_scatter, reached by specular turns only) in column
    0, every other mode in the rest column."""
    t = -np.ones(inp['tau'].shape[0], dtype=np.int32)
    t[inp['P']] = 0
    return t


def _restate_args(inp, fused):
    ct = inp['ct']
    return dict(seed=inp['seed'], max_events=inp['max_events'] or K.MAX_EVENTS, rough=ct['rough'], J=ct['J'], fused=fused)


def run(name, fused=True):
    """The restatement on an edge case, with `trace` (kinetic_cases.restate's counts) added (cached; callers must not modify it)."""
    def make():
        inp = inputs(name)
        ct = inp['ct']
        trace = {}
        with tables_of(inp):
            r = K.restate(ct['mesh'], K.subvols(ct), FC.group_vel(ct), inp['tau'], inp['c'], inp['n'], trace=trace, **_restate_args(inp, fused))
        return dict(r, trace=trace)
    return cached(('kin_edge_run', name, fused), make)


def run_grouped(name):
    """The grouped restatement on an edge case with group_table() (cached)."""
    def make():
        inp = inputs(name)
        ct = inp['ct']
        with tables_of(inp):
            return KGC.restate_grouped(group_table(inp['tau'].shape[0]), 3, ct['mesh'], K.subvols(ct), FC.group_vel(ct), inp['tau'], inp['c'],
                                       inp['n'], **_restate_args(inp, True))
    return cached(('kin_edge_grp', name), make)


def shape_run(n):
    """The restatement on the 'ttp_16' parity inputs with n rays per source."""
    p = K.PARITY['ttp_16']
    return K.run_case(p['case'], n, p['seed'], scale=p['scale'])


def left_out_share(name):
    """The share of rays whose event sequence differs between fused and unfused positions."""
    return float((run(name)['ray_hash'] != run(name, fused=False)['ray_hash']).mean())


def host_rows(r):
    """rows [F, 32] from a result's per-ray outputs at the report's scales and bounds: the ends, the counts, the integer sums the
    device adds -- a term above its bound adds 0 and is counted -- and, in words 20 .. 22, how many of each kind were left out.
    Words 23 and 24 (the segments' terms) are not the rays' to give and are copied from r['rows']."""
    rep = r['report']
    F = r['ends'].shape[0]
    Bx, Bt = rep['B_x'], rep['B_t']
    BD, BD2, BT = 1024.0 * Bx, (32.0 * Bx) * (32.0 * Bx), 1024.0 * Bt
    rows = np.zeros((F, K.ROW_WORDS), dtype=np.int64)
    for f in range(F):
        e = r['ray_end'][f]
        rows[f, :F] = [(e == g).sum() for g in range(F)]
        rows[f, 8:11] = [(e == c).sum() for c in (K.END_LOST, K.END_MISSED, K.END_CAPPED)]
        rows[f, 11], rows[f, 12] = r['ray_events'][f].sum(), r['ray_casts'][f].sum()
        D, T = r['ray_D'][f], r['ray_dwell'][f]
        for a in range(3):
            q, o = K._q(D[:, a], 2.0 ** rep['k_D'], BD)
            rows[f, 13 + a], rows[f, 20] = q.sum(), rows[f, 20] + o
            q, o = K._q(D[:, a] * D[:, a], 2.0 ** rep['k_D2'], BD2)
            rows[f, 16 + a], rows[f, 21] = q.sum(), rows[f, 21] + o
        q, o = K._q(T, 2.0 ** rep['k_T'], BT)
        rows[f, 19], rows[f, 22] = q.sum(), o
        rows[f, 23:25] = r['rows'][f, 23:25]
    return rows
