"""The face tree of the three meshes of tests/test_gpu_tree_edges.py as Engine.tree_info reports it, and the rays outside the slab
test's stated domain (nk_device.h, NK_RAY_BIG): every component below 1e-30 in magnitude, in unequal ratio.  All their 1 / v clamp
to the same value, the slab test follows another direction than the ray's, and the walk misses hits that the all-faces reference
and the plane sweep (NK_NO_TREE=1) find.  Developer probe; profiles/tree_edge_margins.txt quotes its output."""
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import edge_cases as EC  # noqa: E402
from test_gpu_tree_edges import tree_engine  # noqa: E402

for name in ['wire72', 'star', 'longwire']:
    g = EC.tree_mesh(name)
    x, v = EC.subtiny_rays(g)
    ref = EC.all_faces_cast(g, x, v)
    eng = tree_engine(name)
    info = eng.tree_info()
    xc, tc, fc = eng.find_boundary(x, v)
    eng.close()
    print('%s: NG %d, tree_top %d, nodes per level %s, top family %d, %d leaves, %d references (%d faces), %d empty leaf slots, tree_bound %.6g' % (
        name, info['NG'], info['tree_top'], info['level_nodes'], info['top_family'], info['tree_leaves'], info['references'],
        np.asarray(g['face_normals']).shape[0], info['pad_slots'], info['tree_bound']))
    hit = ref['hit']
    print('   subtiny: reference hits %d of %d (t %.3g .. %.3g); the walk misses %d of them, names another facet on %d, another t on %d' % (
        hit.sum(), x.shape[0], ref['tc'][hit].min(), ref['tc'][hit].max(), (hit & (fc < 0)).sum(),
        (hit & (fc >= 0) & (fc != ref['fc'])).sum(), (hit & (fc >= 0) & (tc != ref['tc'])).sum()), flush=True)
