"""CPU: acs_ekf_debug_plan, the host-only view of acs_ekf_run's dispatch (ekf_plan in
csrc/ekf.hip, the function acs_ekf_enqueue launches by), over every parameter count the C ABI
takes, and the parity cases of tests/test_gpu_ekf_sizes.py against it: every filter, gain and
smoother instance any P in 3..32 can select is run by at least one of those cases."""
import pytest

import ekf_sizes as es
from acinoset_amd import _native

W1, WG = 'k_ekf_filter_w1', 'k_ekf_filter'
# P: (npad, filter, waves, gains without P_smooth, state recursion without P_smooth); 12 cameras,
# 8 frames. n = 3P, npad = n rounded up to 16.
TABLE = {}
for _P in range(3, 33):
    _npad = (3 * _P + 15) // 16 * 16
    TABLE[_P] = (_npad, WG, 8, 'k_ekf_gain' if _npad < 48 else f'k_ekf_gain_t<{_npad // 16}>', 'k_ekf_smooth_x')
TABLE[6] = (32, W1, 4, 'k_ekf_gain_w', 'k_ekf_smooth_xs<18,8>')
TABLE[29] = (96, WG, 8, 'k_ekf_gain_t<6>', 'k_ekf_smooth_xs<87,2>')
# the table written out for the sizes of the shipped and the test skeletons and both ends
WRITTEN = {3: (16, WG, 8, 'k_ekf_gain', 'k_ekf_smooth_x'), 5: (16, WG, 8, 'k_ekf_gain', 'k_ekf_smooth_x'),
           6: (32, W1, 4, 'k_ekf_gain_w', 'k_ekf_smooth_xs<18,8>'), 7: (32, WG, 8, 'k_ekf_gain', 'k_ekf_smooth_x'),
           10: (32, WG, 8, 'k_ekf_gain', 'k_ekf_smooth_x'), 11: (48, WG, 8, 'k_ekf_gain_t<3>', 'k_ekf_smooth_x'),
           16: (48, WG, 8, 'k_ekf_gain_t<3>', 'k_ekf_smooth_x'), 17: (64, WG, 8, 'k_ekf_gain_t<4>', 'k_ekf_smooth_x'),
           18: (64, WG, 8, 'k_ekf_gain_t<4>', 'k_ekf_smooth_x'), 21: (64, WG, 8, 'k_ekf_gain_t<4>', 'k_ekf_smooth_x'),
           22: (80, WG, 8, 'k_ekf_gain_t<5>', 'k_ekf_smooth_x'), 26: (80, WG, 8, 'k_ekf_gain_t<5>', 'k_ekf_smooth_x'),
           27: (96, WG, 8, 'k_ekf_gain_t<6>', 'k_ekf_smooth_x'), 28: (96, WG, 8, 'k_ekf_gain_t<6>', 'k_ekf_smooth_x'),
           29: (96, WG, 8, 'k_ekf_gain_t<6>', 'k_ekf_smooth_xs<87,2>'),
           30: (96, WG, 8, 'k_ekf_gain_t<6>', 'k_ekf_smooth_x'), 32: (96, WG, 8, 'k_ekf_gain_t<6>', 'k_ekf_smooth_x')}


def _row(p):
    return (p['npad'], p['filter'], p['waves'], p['gains'], p['smoother'])


def test_written_table_is_the_rule():
    assert all(TABLE[P] == row for P, row in WRITTEN.items())


@pytest.mark.parametrize('P', range(3, 33))
def test_ekf_plan_every_parameter_count(P):
    """A chain-like table of P parameters (3 markers, 4 nodes, one joint per 3 angles) on 12
    cameras: the dispatch by P alone."""
    kw = dict(n_joints=max(1, (P - 3) // 3), n_nodes=4)
    p = _native.ekf_debug_plan(P, es.N_CAMS, 3, es.N_FRAMES, **kw)
    assert _row(p) == TABLE[P], p
    assert 0 < p['lds'] <= (64 if P == 6 else 160) * 1024
    # with P_smooth: the sequential smoother forms its own gains, at every size
    q = _native.ekf_debug_plan(P, es.N_CAMS, 3, es.N_FRAMES, covariances=True, **kw)
    assert _row(q) == TABLE[P][:3] + ('none', 'k_ekf_smooth') and q['lds'] == p['lds']
    # one frame: no gain, the same recursion kernel (it copies the last filtered state)
    one = _native.ekf_debug_plan(P, es.N_CAMS, 3, 1, **kw)
    assert _row(one) == TABLE[P][:3] + ('none', TABLE[P][4])
    assert _row(_native.ekf_debug_plan(P, es.N_CAMS, 3, 2, **kw)) == TABLE[P]


def test_ekf_plan_lds_of_the_shipped_tables():
    """The filter's LDS grows with the table and the cameras; the head model leaves the
    small-state kernel when its LDS passes 64 KB (the cameras decide)."""
    lds = {m: _native.ekf_debug_plan(es.case(m).table, es.N_CAMS, 0, es.N_FRAMES)['lds'] for m in es.SIZES}
    assert lds['head'] < lds['neck10'] < lds['upper_body'] < lds['front18'] < lds['default_nolure'] < lds['default']
    assert lds['head_stabilize'] < lds['upper_body'] and lds['default'] <= 160 * 1024
    head = es.case('head').table
    by_cams = [_native.ekf_debug_plan(head, c, 0, 8) for c in range(1, 65)]
    assert all(a['lds'] < b['lds'] for a, b in zip(by_cams, by_cams[1:]) if a['filter'] == b['filter'])
    assert by_cams[0]['filter'] == by_cams[31]['filter'] == W1      # the 24 / 32-camera rings of test_gpu_ekf.py
    for p in by_cams:
        assert (p['filter'], p['waves']) == ((W1, 4) if p['filter'] == W1 and p['lds'] <= 65536 else (WG, 8))
        assert p['gains'] == 'k_ekf_gain_w' and p['smoother'] == 'k_ekf_smooth_xs<18,8>'
    w1 = [p['filter'] == W1 for p in by_cams]
    assert w1 == sorted(w1, reverse=True)                            # one switch, upwards in cameras


def test_ekf_plan_refuses_what_the_run_refuses():
    ok = dict(P=26, n_cams=12, L=20, n_frames=8, n_joints=14, n_nodes=21)
    _native.ekf_debug_plan(**ok)
    for kw in (dict(P=2), dict(P=33), dict(n_cams=0), dict(n_cams=65), dict(n_frames=0), dict(L=0), dict(L=22),
               dict(n_joints=0), dict(n_joints=17), dict(n_nodes=33, L=33)):
        with pytest.raises(ValueError):
            _native.ekf_debug_plan(**dict(ok, **kw))
    # LDS over 160 KB: the largest table the FK takes (16 joints, 32 nodes, 32 markers), at any
    # camera count; 32 parameters on a tree of the shipped size fit, on 64 cameras too
    big = dict(P=32, n_cams=1, L=32, n_frames=8, n_joints=16, n_nodes=32)
    with pytest.raises(ValueError):
        _native.ekf_debug_plan(**big)
    assert 150 * 1024 < _native.ekf_debug_plan(**dict(big, n_cams=64, L=20, n_joints=14, n_nodes=22))['lds'] \
        <= 160 * 1024


def test_parity_cases_reach_every_instance():
    """The sizes of tests/test_gpu_ekf_sizes.py, each run with and without P_smooth, select every
    filter, gain and smoother value that any P in 3..32 selects (any table, any camera count)."""
    possible = {k: set() for k in ('filter', 'gains', 'smoother')}
    for P in range(3, 33):
        for n_cams in (1, 12, 64):
            for N in (1, 8):
                for cov in (False, True):
                    try:
                        p = _native.ekf_debug_plan(P, n_cams, 3, N, covariances=cov, n_nodes=4)
                    except ValueError:
                        continue
                    for k in possible:
                        possible[k].add(p[k])
    assert possible['filter'] == set(_native.EKF_FILTERS) and possible['gains'] == set(_native.EKF_GAINS)
    assert possible['smoother'] == set(_native.EKF_SMOOTHERS)
    reached = {k: set() for k in possible}
    npads = set()
    for name in es.SIZES:
        t = es.case(name).table
        for N, cov in ((es.N_FRAMES, False), (es.N_FRAMES, True), (1, False)):   # N = 1: the shortest clips
            p = _native.ekf_debug_plan(t, es.N_CAMS, 0, N, covariances=cov)
            npads.add(p['npad'])
            for k in reached:
                reached[k].add(p[k])
    assert reached == possible, {k: possible[k] - reached[k] for k in possible}
    assert npads == {32, 48, 64, 80, 96}
    want = {'head': 6, 'neck10': 10, 'upper_body': 11, 'head_stabilize': 11, 'front18': 18, 'default_nolure': 26,
            'default': 29}
    assert {n: es.case(n).table.P for n in es.SIZES} == want
    # the two 11-parameter tables differ in their nodes (8 / 6) and markers (7 / 5)
    ub, hs = es.case('upper_body').table, es.case('head_stabilize').table
    assert (ub.n_nodes, ub.L, hs.n_nodes, hs.L) == (8, 7, 6, 5)
