"""The emulation of the wave-cooperative scenario generator's shortcuts (generator_window_emulation.py) against the plain
sequential form of the reference's rejection sampling: this file pins the ALGORITHM on machines without a GPU."""
import numpy as np
import pytest

from generator_window_emulation import (
    F, PI, TRIG_ABS_ERROR, BlockedGrid, attempts_of, collides, float32_position, position, prefilter_margin, sequential, table_margin,
    windowed, windowed_table)


@pytest.mark.parametrize('R,humans,cap', [(12.0, 20, 1 << 23), (4.0, 12, 1 << 23), (3.0, 9, 1 << 23), (2.6, 8, 256), (2.2, 8, 128),
                                          (2.0, 7, 64), (2.0, 9, 100), (1.6, 6, 64)])
def test_window_reuse_places_every_human_where_the_sequential_loop_does(R, humans, cap):
    v_pref, min_dist = 1.0, 0.3 + 0.3 + 0.2
    gave_up = 0
    fewer = 0
    for seed in range(40):
        att = attempts_of(1000 + seed, 400000 if cap > 1000 else 20000)
        try:
            want, cur, err = sequential(att, humans, R, v_pref, min_dist, cap)
        except IndexError:  # a crowding this seed does not get out of within the attempts drawn here
            continue
        got, cur2, err2, windows = windowed(att, humans, R, v_pref, min_dist, cap)
        assert cur2 == cur and err2 == err
        assert np.array_equal(np.array(got), np.array(want))
        gave_up += err
        fewer += windows < humans
    if cap <= 256:
        assert gave_up > 0  # the give-up rule was exercised
    if R >= 12.0:
        assert fewer == 40  # an easy scenario takes fewer window evaluations than it has humans


@pytest.mark.parametrize('R', [4.0, 12.0, 40.0])
def test_float32_prefilter_rejects_only_what_the_exact_test_rejects(R):
    rng = np.random.RandomState(7)
    v_pref, min_dist = 1.0, 0.8
    margin = prefilter_margin(R)
    # 20 placed humans on the circle (positions and goals), as the generator would have them
    ang = rng.uniform(0, 2 * PI, 20)
    placed = [(R * np.cos(a) + rng.uniform(-.5, .5), R * np.sin(a) + rng.uniform(-.5, .5)) for a in ang]
    placed = [(px, py, -px, -py) for px, py in placed]
    words = rng.randint(0, 2 ** 32, size=(1000000, 6), dtype=np.uint64)
    # the exact path: np.random.random() from two words each (random_at)
    u = ((words[:, 0::2] >> 5).astype(np.float64) * 67108864.0 + (words[:, 1::2] >> 6).astype(np.float64)) / 9007199254740992.0
    x, y = position(u, R, v_pref)
    exact = collides(x, y, placed, min_dist)
    # the prefilter: the first word's top 27 bits, float32 throughout (scenario_wave.h)
    f = ((words[:, 0::2] >> 5).astype(np.float32) * np.float32(2.0 ** -27))
    a32 = f[:, 0] * np.float32(6.2831855)
    # (the device's V_COS_F32 / V_SIN_F32 are within kTrigAbsError of the true values: the worst case, both off by the bound)
    sign = np.where(rng.randint(0, 2, size=(len(f), 2)) > 0, np.float32(1), np.float32(-1)) * np.float32(TRIG_ABS_ERROR)
    fx = np.float32(R) * (np.cos(a32, dtype=np.float32) + sign[:, 0]) + (f[:, 1] - np.float32(0.5)) * np.float32(v_pref)
    fy = np.float32(R) * (np.sin(a32, dtype=np.float32) + sign[:, 1]) + (f[:, 2] - np.float32(0.5)) * np.float32(v_pref)
    t = np.float32(min_dist) - margin
    inside = np.zeros(len(fx), bool)
    for px, py, gx, gy in placed:
        for qx, qy in ((np.float32(px), np.float32(py)), (np.float32(gx), np.float32(gy))):
            ax, ay = fx - qx, fy - qy
            inside |= (ax * ax + ay * ay) < t * t
    assert not np.any(inside & ~exact)          # conservative
    assert inside.sum() > 0.98 * exact.sum()    # and it catches nearly everything the exact test rejects
    # the float32 position is well inside the bound the margin was derived from (margin = 10 x the bound)
    assert np.max(np.hypot(fx.astype(np.float64) - x, fy.astype(np.float64) - y)) < 0.2 * float(margin)


@pytest.mark.parametrize('R', [2.0, 4.0, 12.0])
def test_blocked_cell_table_rejects_only_what_the_exact_test_rejects(R):
    rng = np.random.RandomState(11)
    v_pref, min_dist = 1.0, 0.8
    ang = rng.uniform(0, 2 * PI, 20)
    placed = [(R * np.cos(a) + rng.uniform(-.5, .5), R * np.sin(a) + rng.uniform(-.5, .5)) for a in ang]
    placed = [(0.0, -R, 0.0, R)] + [(px, py, -px, -py) for px, py in placed]
    grid = BlockedGrid(R, v_pref)
    for px, py, gx, gy in placed:
        grid.mark(px, py, F(min_dist) - table_margin(R))
        grid.mark(gx, gy, F(min_dist) - table_margin(R))
    att = rng.random_sample((1000000, 3))
    x, y = position(att, R, v_pref)
    exact = collides(x, y, placed, min_dist)
    fx, fy = float32_position(att, R, v_pref, rng)
    blocked = grid.blocked(fx, fy)
    assert not np.any(blocked & ~exact)   # conservative: every table rejection is an exact rejection
    if R == 4.0:
        assert blocked.sum() > 0.97 * exact.sum()   # the reference geometry: nearly every rejection is decided by one bit
    # a set cell lies within min_dist of its disc's centre even after the float32 position's error: check the corners
    iy, ix = np.nonzero(grid.bits)
    x0, y0 = ix * float(grid.cell) - float(grid.ext), iy * float(grid.cell) - float(grid.ext)
    slack = 0.5 * float(table_margin(R))
    for dx in (-slack, float(grid.cell) + slack):
        for dy in (-slack, float(grid.cell) + slack):
            assert collides(x0 + dx, y0 + dy, placed, min_dist).all()


@pytest.mark.parametrize('R,humans,cap', [(12.0, 20, 1 << 23), (4.0, 14, 1 << 23), (3.0, 9, 1 << 23), (2.6, 8, 256), (2.2, 8, 128),
                                          (2.0, 7, 64), (2.0, 9, 100)])
def test_table_generator_places_every_human_where_the_sequential_loop_does(R, humans, cap):
    v_pref, min_dist = 1.0, 0.3 + 0.3 + 0.2
    gave_up, surv, exact, windows = 0, 0, 0, 0
    for seed in range(40):
        att = attempts_of(1000 + seed, 400000 if cap > 1000 else 20000)
        try:
            want, cur, err = sequential(att, humans, R, v_pref, min_dist, cap)
        except IndexError:
            continue
        got, cur2, err2, st = windowed_table(att, humans, R, v_pref, min_dist, cap)
        assert cur2 == cur and err2 == err
        assert np.array_equal(np.array(got), np.array(want))
        gave_up += err
        surv, exact, windows = surv + st['survivors'], exact + st['exact'], windows + st['windows']
    if cap <= 256:
        assert gave_up > 0
    if R == 4.0:   # crowded: the table leaves well under one survivor per window, and most survivors die in float32
        assert surv < windows + 2 * 40 * humans and exact <= surv
