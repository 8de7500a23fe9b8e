"""CPU: acs_fte_debug_plan, the host-only restatement-free view of the FTE solve's dispatch
(fte_shape, lin_kernel, cr_asm_threads, cr_level_counts, cr_nsplit, cr_level_deep), on a
256-CU device: the size-selected paths of DESIGN's table. `3w` = nsplit 3 on the
one-wave-per-column-block (upper-tile) path, `5D` = nsplit 5 on the deep (full-tile) path."""
import pytest

from acinoset_amd import _native, kinematics as pkin

P = {m: pkin.build_table(m).P for m in ('head', 'upper_body', 'default_nolure', 'default')}


def _seq(plan, n):
    return ' '.join(f"{ns}{'D' if deep else 'w'}" for _, _, ns, deep in plan['levels'][:n])


TABLE = [
    # mode, cameras, {N: first levels}
    ('head', 6, {389: '3D 5D 5D', 771: '1w 2w 5D 5D', 1537: '1w 1w 2w 5D 5D'}),
    ('head', 16, {389: '3D 6D 6D', 771: '1w 2w 6D 6D', 1537: '1w 1w 2w 6D 6D'}),
    ('upper_body', 6, {389: '3D 6D 7D 7D', 771: '1w 2w 6D 7D 7D', 1537: '1w 1w 2w 6D 7D'}),
    ('upper_body', 16, {389: '3D 6D 8D 8D', 771: '1w 2w 6D 8D 8D', 1537: '1w 1w 2w 6D 8D'}),
    ('default_nolure', 6, {389: '3D 6D 11D 11D', 771: '1w 2w 6D 11D 11D', 1537: '1w 1w 2w 6D 11D'}),
    ('default_nolure', 16, {389: '3D 6D 12D 12D', 771: '2w 2w 6D 12D 12D', 1537: '2w 2w 2w 6D 12D'}),
    ('default', 6, {389: '3w 6D 13D 13D', 771: '2w 2w 6D 13D', 1537: '2w 2w 2w 6D 13D'}),
    ('default', 16, {389: '3w 6D 14D 14D', 771: '2w 2w 6D 14D', 1537: '2w 2w 2w 6D 14D'}),
]


@pytest.mark.parametrize('mode,n_cams,rows', TABLE, ids=[f'{m}-{c}' for m, c, _ in TABLE])
def test_fte_plan_levels_on_256_cus(mode, n_cams, rows):
    BP = {'head': 32, 'upper_body': 48, 'default_nolure': 80, 'default': 96}[mode]
    for N, want in rows.items():
        p = _native.fte_debug_plan(N, P[mode], n_cams, n_cu=256)
        assert (p['BP'], p['GR'], p['Cg']) == (BP, 32 if n_cams == 16 else 16, n_cams), p
        assert p['nblk'] == (N + 4) // 3 and 1 << p['nlev'] >= p['nblk'] > 1 << (p['nlev'] - 1), p
        assert _seq(p, len(want.split())) == want, (N, _seq(p, 6))
        # level 0 eliminates the odd blocks and has no survivor workgroups; later levels halve
        ne0, ns0 = p['levels'][0][:2]
        assert (ne0, ns0) == (p['nblk'] // 2, 0)
        assert p['levels'][1][:2] == ((p['nblk'] + 1) // 4, (p['nblk'] + 3) // 4)
        assert p['levels'][-1][0] == 1
        assert p['d_upper'] == (1 if n_cams < 16 else 0)


def test_fte_plan_assembly_and_linearize_thresholds():
    """The 512-thread compact-row assembly past two rounds of 1,024-thread blocks per CU (the
    given CU count, not a process-wide one); k_fte_linearize<5> past 1,024 frames."""
    for n_cu, first in ((256, 1535), (304, 1823), (64, 383)):
        assert first == 3 * (2 * n_cu + 1) - 4
        assert _native.fte_debug_plan(first - 1, P['head'], 6, n_cu=n_cu)['asm'] == 1024
        assert _native.fte_debug_plan(first, P['head'], 6, n_cu=n_cu)['asm'] == 512
    assert _native.fte_debug_plan(1024, P['default'], 16, n_cu=256)['lin'] == 4
    assert _native.fte_debug_plan(1025, P['default'], 16, n_cu=256)['lin'] == 5


def test_fte_plan_delay_modes():
    """Variable delays: no constant-delay border (Cg = 0, GR = 16), k_fte_assemble + k_cr_build
    (asm 0), D stored whole; no delay: Cg = 0 through k_cr_assemble_build, D as upper tiles."""
    v = _native.fte_debug_plan(771, P['default_nolure'], 16, sd_mode='variable', n_cu=256)
    assert (v['Cg'], v['GR'], v['asm'], v['d_upper']) == (0, 16, 0, 0)
    n = _native.fte_debug_plan(771, P['default_nolure'], 16, shutter_delay=False, n_cu=256)
    assert (n['Cg'], n['GR'], n['asm'], n['d_upper']) == (0, 16, 1024, 1)
    assert v['levels'] == n['levels'] == _native.fte_debug_plan(771, P['default_nolure'], 6, n_cu=256)['levels']


def test_fte_plan_rejects_bad_arguments():
    for kw in (dict(n_frames=1), dict(P=2), dict(P=33), dict(n_cams=0), dict(n_cams=17), dict(n_cu=0)):
        a = dict(n_frames=100, P=26, n_cams=6, n_cu=256)
        a.update(kw)
        with pytest.raises(ValueError):
            _native.fte_debug_plan(**a)
