"""Host side of the stream pool (tinyrecurrentunet_amd/streaming.py): the planner that decides which rows, which frame, which
envelope and which pass, and the slot allocator.  Plain host code: no pool, no device, no library."""
import itertools
import os
import subprocess
import sys

import pytest

from tinyrecurrentunet_amd import streaming as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_planner_and_the_allocator_need_no_library():
    """in a fresh interpreter: planning and allocating load neither libtrunet_hip.so nor a device"""
    code = ("from tinyrecurrentunet_amd import streaming as st, _lib\n"
            "import torch\n"
            "st.plan_step([0, 3, 7], [0, 2]); st.plan_close([3], [5]); st.SlotAllocator(4).open(2)\n"
            "assert _lib._lib is None and not torch.cuda.is_initialized()\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr


def test_hop_env_counts_the_covering_frames():
    # open session: hop 0 is covered by frames 0..2, every later hop by four
    assert [int(st.hop_env(k)) for k in range(4)] == [3, 4, 4, 4]
    # an utterance of T frames: the last whole hop (T - 2) has three, as torch.istft's rectangular envelope does
    assert st.hop_env(0, 3) == 3 and st.hop_env(8, 11) == 4 and st.hop_env(9, 11) == 3


@pytest.mark.parametrize("listed", [c for n in range(8) for c in itertools.combinations(range(7), n)])
def test_plan_step_follows_the_latency_table(listed):
    """slot s has received s hops (0..6); every subset of the slots is listed.  After the step a session has a = s + 1 hops:
    a = 1, 2: the hop is stored; a = 3: frames 0 and 1 in passes 1 and 2, nothing delivered; a >= 4: frame a - 2 in pass 1,
    output hop a - 4 with the envelope of an interior hop (3 for hop 0)."""
    hops = list(range(7))
    listed = list(listed)
    plan = st.plan_step(hops, listed)
    assert hops == list(range(7))                                   # the planner does not touch its input
    assert plan.valid.tolist() == [hops[s] + 1 >= 4 for s in listed]
    assert plan.hops.tolist() == [hops[s] + 1 for s in listed]
    assert len(plan.tables) <= 2 and len(plan.frames) == len(plan.tables)
    assert all(t.shape[1] == st.ROW_INTS and t.dtype.name == "int32" and len(t) > 0 for t in plan.tables)
    third = [s for s in listed if hops[s] + 1 == 3]
    assert len(plan.tables) == (2 if third else (1 if listed else 0))
    t1 = st.rows_of(plan.tables[0]) if plan.tables else []
    p1, stores = t1[:plan.frames[0]] if plan.tables else [], t1[plan.frames[0]:] if plan.tables else []
    p2 = st.rows_of(plan.tables[1]) if third else []
    if third:
        assert plan.frames[1] == len(p2)
    assert [(w.slot, w.pos) for w in stores] == [(s, i) for i, s in enumerate(listed) if hops[s] + 1 < 3]
    for w in stores:
        assert w.flags == st.ROW_SHIFT | st.ROW_NOFRAME and w.out == -1 and w.hops == hops[w.slot] + 1
    assert [w.slot for w in p1] == [s for s in listed if hops[s] + 1 >= 3]
    assert [w.slot for w in p2] == third
    for w in p1:
        a = hops[w.slot] + 1
        assert w.hops == a and w.tail == 0 and listed[w.pos] == w.slot
        if a == 3:
            assert (w.flags, w.frame, w.env, w.out) == (st.ROW_SHIFT | st.ROW_FIRST, 0, 1, -1)
        else:
            assert (w.flags, w.frame, w.out) == (st.ROW_SHIFT, a - 2, w.pos)
            assert w.env == (3 if a == 4 else 4)
    for w in p2:
        assert (w.flags, w.frame, w.env, w.out, w.hops, w.tail) == (st.ROW_STASHED, 1, 2, -1, 3, 0)
        assert listed[w.pos] == w.slot
    # unlisted slots appear nowhere
    assert {w.slot for w in t1 + p2} == set(listed)


@pytest.mark.parametrize("a,r", [(2, 1), (2, 127), (3, 0), (3, 5), (10, 0), (10, 64), (10, 127)])
def test_plan_close_computes_the_missing_frames_and_all_remaining_samples(a, r):
    L = 128 * a + r
    T = 1 + L // 128
    plan = st.plan_close([a], [r])
    assert all(len(t) == 1 for t in plan.tables) and len(plan.tables) <= 3 and plan.frames == [1] * len(plan.tables)
    rows = [st.rows_of(t)[0] for t in plan.tables]
    done = a - 1 if a >= 3 else 0                         # frames computed by the steps: 0 .. a - 2 from the third hop on
    assert [w.frame for w in rows] == list(range(done, T))
    assert done + len(rows) == T
    assert plan.lengths == [L - 128 * max(a - 3, 0)]
    assert 128 * max(a - 3, 0) + plan.lengths[0] == L      # delivered by the steps + returned by close = L samples
    assert all(w.tail == r and w.hops == a and not w.flags & (st.ROW_SHIFT | st.ROW_NOFRAME) for w in rows)
    assert [bool(w.flags & st.ROW_FINISH) for w in rows] == [False] * (len(rows) - 1) + [True]
    assert [bool(w.flags & st.ROW_FIRST) for w in rows] == [w.frame == 0 for w in rows]
    # frame 1 is transformed together with frame 0 (one complex FFT, as the offline kernels pair them) and only fetched
    assert [bool(w.flags & st.ROW_STASHED) for w in rows] == [w.frame == 1 for w in rows]
    if a == 2:
        # frames 0 and 1 complete centre padding only; frame 2 completes hop 0 (3 frames), then hop 1 (3) and the tail (2)
        assert [w.out for w in rows] == [-1, -1, 0] and rows[2].env == 3
        assert plan.lengths[0] == 128 + 128 + r
    else:
        assert [w.out for w in rows] == [0, 1]
        assert rows[0].env == (3 if a == 3 else 4) and rows[1].env == 4
        assert plan.lengths[0] == 128 + 128 + 128 + r      # hops a - 3, a - 2, a - 1 (3 frames) and the tail (2 frames)


@pytest.mark.parametrize("a,r", [(2, 0), (1, 100), (0, 50)])
def test_plan_close_refuses_utterances_below_257_samples(a, r):
    with pytest.raises(ValueError):
        st.plan_close([10, a], [0, r])


def test_plan_close_lays_sessions_out_side_by_side():
    plan = st.plan_close([2, 5, 3], [7, 0, 127], slots=[4, 0, 9])
    rows = [st.rows_of(t) for t in plan.tables]
    assert [[w.slot for w in p] for p in rows] == [[4, 0, 9], [4, 0, 9], [4]]
    assert [[w.pos for w in p] for p in rows] == [[0, 1, 2], [0, 1, 2], [0]]
    assert [[w.out for w in p] for p in rows] == [[-1, 4, 8], [-1, 5, 9], [0]]
    assert plan.lengths == [263, 384, 511]
    with pytest.raises(ValueError):
        st.plan_close([5], [128])
    with pytest.raises(ValueError):
        st.plan_close([5], [-1])


def test_a_session_of_any_age_plans_like_a_young_one():
    young, old = st.plan_step([5, 2], [0, 1]), st.plan_step([10 ** 8, 2], [0, 1])
    d = old.tables[0].astype("int64") - young.tables[0]
    assert d[0].tolist() == [0, 0, 10 ** 8 - 5, 10 ** 8 - 5, 0, 0, 0, 0] and not d[1].any()   # frame and hops move together


def test_slot_allocator():
    al = st.SlotAllocator(5)
    assert (al.capacity, al.free) == (5, 5)
    a = al.open(2)
    b = al.open(3)
    assert sorted(a + b) == list(range(5)) and al.free == 0
    with pytest.raises(Exception):
        al.open(1)                                       # full
    assert al.free == 0 and al.is_open.all()
    al.release([b[0], a[1]])
    assert al.free == 2 and not al.is_open[b[0]]
    with pytest.raises(ValueError):
        al.release([b[0]])                               # not open
    with pytest.raises(ValueError):
        al.release([a[0], a[0]])                         # twice
    assert al.free == 2 and al.is_open[a[0]]
    with pytest.raises(Exception):
        al.open(3)                                       # only two are free: nothing is handed out
    assert al.free == 2
    c = al.open(2)
    assert sorted(c) == sorted([b[0], a[1]])             # reused ...
    al2 = st.SlotAllocator(8)
    live = []
    import random
    rng = random.Random(0)
    for _ in range(200):                                 # ... and never out twice
        if live and (rng.random() < 0.5 or al2.free == 0):
            i = live.pop(rng.randrange(len(live)))
            al2.release([i])
        else:
            (i,) = al2.open(1)
            assert i not in live
            live.append(i)
        assert al2.free + len(live) == 8
    with pytest.raises(ValueError):
        st.SlotAllocator(0)
