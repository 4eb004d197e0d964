"""batch_play_kernel (csrc/batch_play.hip): the steps of a batch call in ONE launch, every member's velocity kept in LDS
from step to step.  sfl_batch_step_n and sfl_batch_step_n_each take it on a batch of sfl_batch_create when n >= 2 and the
timeline of queued forces (include/sfl.h, "the timeline rule") holds a record for some step of [1, n).

The yardstick is code that existed before: a twin batch stepped one step at a time by the per-step kernels, with that
step's records queued by the old step-0 call in front of each step -- and the oracle's operators.  All four fields (velocity,
divergence, pressure, dye) are compared bit for bit, the update norm too.  The state is handed from the per-step kernels to
the play kernel and back: one old step in front of the call under test, old steps behind it."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from test_batch import DT, FIELDS, OMEGA, download_all, member_fields, upload_members
from test_batch_frames import render_each
from test_force_timeline import assert_batches_equal, batch_script, oracle_steps, queue_batch

BATCH = 3
SHAPES = [(2, 2), (3, 2), (7, 9), (61, 81), (64, 96)]   # no interior cell (2); more than one pass of 1024 threads; 6144 cells: the LDS limit
PARAMS = ([DT, DT / 2, DT * 2], [1.0, 0.5, 2.0], [0, 3, 5], [1.96, 1.5, 1.9])   # dt, dx, iters, omega of the three members


def play_case(sfl, oracle, dim_x, dim_y, n, each, iters=4):
    fields = [member_fields(dim_x, dim_y, 500 + 10 * n + m, 40.0) for m in range(BATCH)]
    sc = batch_script(n, dim_x, dim_y)
    prm = sfl.member_params(BATCH, *PARAMS) if each else None
    if each and iters != 4:
        prm["iters"] = iters
    step = (lambda x, k: x.step_n_each(k, prm)) if each else (lambda x, k: x.step_n(k, DT, 1.0, iters, OMEGA))
    with sfl.BatchSolver(dim_x, dim_y, BATCH) as b, sfl.BatchSolver(dim_x, dim_y, BATCH) as twin:
        upload_members(b, fields), upload_members(twin, fields)
        step(b, 1), step(twin, 1)                          # per-step kernels -> play kernel
        start = download_all(twin)
        for k in sorted(sc, reverse=True):                 # steps in an order of their own; step 0 by the old call
            queue_batch(b, sc[k], None if k == 0 else k)
        assert b.forces_pending() == (sum(len(r) for r in sc.values()), n + 2)
        step(b, n)                                         # the call under test: one launch
        assert b.forces_pending() == (1, 2)
        for k in range(n):
            queue_batch(twin, sc.get(k))
            step(twin, 1)
        got = download_all(b)
        for name, a, w in zip(FIELDS, got, download_all(twin)):
            assert_bit_equal(a, w, f"{name} after {n} steps in one launch against one launch per step")
        if each:
            assert_bit_equal(b.residual(), twin.residual(), "the update norm of the last step's solve")
        for m in range(BATCH):                             # ... and against the oracle's operators
            records = {k: [(cell, vel) for mm, cell, vel in r if mm == m] for k, r in sc.items()}
            dt, dx, it, om = (prm[m]["dt"], float(prm[m]["dx"]), int(prm[m]["iters"]), prm[m]["omega"]) if each else (DT, 1.0, iters, OMEGA)
            want = oracle_steps(oracle, start[0][m], start[3][m], records, n, dt, dx, it, om)
            for name, a, w in zip(FIELDS, got, want):
                assert_bit_equal(a[m], w, f"{name}, member {m} against the oracle")
        step(b, 2)                                         # play kernel -> per-step kernels: no record in steps 0 and 1
        step(twin, 1), step(twin, 1)
        assert_batches_equal(b, twin, "two steps by the per-step kernels behind the launch")
        assert b.forces_pending() == (1, 0)
        step(b, 1)                                         # the record queued for step n + 2 lands here
        queue_batch(twin, sc[n + 2])
        step(twin, 1)
        assert_batches_equal(b, twin, "the step of the record that survived the call")
        assert b.forces_pending() == (0, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 5])
@pytest.mark.parametrize("dim_x,dim_y", SHAPES)
def test_members_with_parameters_of_their_own(sfl, oracle, dim_x, dim_y, n):
    play_case(sfl, oracle, dim_x, dim_y, n, each=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 5])
@pytest.mark.parametrize("dim_x,dim_y", SHAPES)
def test_uniform_parameters(sfl, oracle, dim_x, dim_y, n):
    play_case(sfl, oracle, dim_x, dim_y, n, each=False)


@pytest.mark.gpu
@pytest.mark.parametrize("each", [False, True])
def test_twenty_iterations_at_the_sketch_shape(sfl, oracle, each):
    play_case(sfl, oracle, 61, 81, 3, each=each, iters=20)


@pytest.mark.gpu
def test_a_recorder_cuts_the_launch_at_the_frames(sfl):
    dim_x, dim_y, n, iters = 61, 81, 5, 4
    fields = [member_fields(dim_x, dim_y, 700 + m, 40.0) for m in range(BATCH)]
    sc = batch_script(n, dim_x, dim_y)
    with sfl.BatchSolver(dim_x, dim_y, BATCH) as b, sfl.BatchSolver(dim_x, dim_y, BATCH) as twin:
        upload_members(b, fields), upload_members(twin, fields)
        b.record_start(every=2, capacity=3)
        for k, records in sc.items():
            queue_batch(b, records, k)
        b.step_n(n, DT, 1.0, iters, OMEGA)
        assert b.record_info() == (2, 3, 5)
        assert b.forces_pending() == (1, 2)
        want = []
        for k in range(n):
            queue_batch(twin, sc.get(k))
            twin.step_n(1, DT, 1.0, iters, OMEGA)
            if k % 2 == 1:
                want.append(render_each(twin))
        assert_bit_equal(b.frames(), np.stack(want), "the frames after steps 2 and 4")
        assert_batches_equal(b, twin, "after five recorded steps")
        # one frame is free; four more steps would complete two: refused, the timeline as it was
        queue_batch(b, [(1, (5, 5), (9.0, 9.0))], 1)
        assert b.forces_pending() == (2, 2)
        with pytest.raises(sfl.SflError) as e:
            b.step_n(4, DT, 1.0, iters, OMEGA)
        assert e.value.code == sfl.capi.ERR_STATE
        assert b.forces_pending() == (2, 2) and b.record_info() == (2, 3, 5)
        assert_batches_equal(b, twin, "nothing stepped")
