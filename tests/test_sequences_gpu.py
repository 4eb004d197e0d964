"""The call sequences of tests/sequence_model.py on the library: one live handle per sequence -- a whole-domain context on
the general kernels, with the fused step boundaries and on the one-workgroup path, a group of three virtual ranks, a
small and a large batch -- taken through 30 seeded ops and compared with the model bit for bit, in three modes over the
same op list: every field after every op (eager), nothing read before the end (lazy), one seeded query after every op
(probing).  tests/test_sequences.py has the census of what the lists contain.

Two more subjects walk solids and histories, 36 ops each: a context (130 x 70: 3 x 3 ragged tiles of the masked solve and,
cleared, the general kernels and the step seams; 61 x 81: cleared, the one-launch step of a small grid) and a batch of three
(61 x 81, 7 x 9) on which a mask is set, replaced without a clear and cleared while the fields stay as they are, with options
flipped, a timeline pending, tracers following, a trail and a history on.  A call the header refuses is an op like any other:
both sides return the refusal, and the fields, the timeline and the tracers behind it are compared as after every op.

Two more walk the viscosity and the loads on top of that vocabulary, 50 and 48 ops each: a context (130 x 70: 3 x 3 ragged
diffusion tiles; 61 x 81: one tile column) and a batch of three (61 x 81, 7 x 9).  The diffusion runs as an operator of one, two
and three launches -- its result in the step's second buffer, in the third, in the second again -- with a reader of the velocity
right behind it; a viscosity is set, cleared and set again while masks come and go, and cleared it gives the step seams, the
one-launch step of a small grid and the unfused step back; a history, a trail and a loads recorder sample behind viscous steps;
a batch stages its coefficient table for step calls queued back to back under a per-member nu with a member at 0; labels are
set before the mask, masks replaced and cleared under labels, labels replaced and reset; a loads recorder counts across calls
that leave remainders, is restarted while on, samples zeros where no mask is set -- inside a context's seam loop and a
batch's one-launch replay -- and, full, refuses a step call whole behind a history and a trail that have room.

Four more walk what came after, at the same shapes.  record-context and record-batch (69 and 76 ops, on the viscous vocabulary):
a history, the loads, the friction, the torque and the averages on at once with five periods across calls that leave remainders;
a full friction and a full torque recorder refusing a call whole; restarts while on; set_bodies refused under either recorder;
pivots kept by the same number of bodies and put back by another, changed while recording, refused with SFL_ERR_INVALID for
another `bodies`; averages that cut a batch's one-launch replay and a context's seams while every >= 1, keep them with
every == 0 and give them back when stopped; float64 planes compared as their bit patterns.  open-context and open-batch (60 and
67 ops, on the solids' vocabulary): a map before and behind a mask, masks replaced and cleared behind a map, inflow cells that go
solid and come back with a profile record on them, set_inflow with and without a profile, a new map that drops the profile, force
records on inflow, profiled and outflow cells, every operator under a map, every plain path behind a cleared map, and the
refusals between openings, viscosity, a history, the divergence view and the calls to a tolerance.

A failure prints the seed, the mode, the first op that disagreed and the op list up to there as a literal for
sequence_model.replay.  There is no tolerance anywhere."""
import functools

import pytest

import sequence_model as sm
from oracle import loader

CASES = [(s.name, case) for s in sm.SUBJECTS for case in s.cases]


@functools.lru_cache(maxsize=None)
def sequences(name):
    subject = next(s for s in sm.SUBJECTS if s.name == name)
    return subject, sm.generate(subject, loader.port())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sm.MODES)
@pytest.mark.parametrize("name,case", CASES, ids=[f"{n}-{c[0]}x{c[1]}-seed{c[2]}" for n, c in CASES])
def test_a_sequence_on_a_live_handle(sfl, oracle, name, case, mode):
    subject, seqs = sequences(name)
    sm.run(subject, case, seqs[case], mode, oracle, lambda s, c: s.library(sfl, c))


LIVE = [(cls, "general") for cls in sm.STAND_INS] + [(cls, "solid-context") for cls in sm.SOLID_STAND_INS]
LIVE += [(cls, sm.stand_in_subject(cls)) for cls in sm.VISCOUS_STAND_INS + sm.LOAD_STAND_INS]      # (viscous-context; viscous-batch for the batch's fault)
LIVE += [(cls, sm.later_stand_in_subject(cls)) for cls in sm.RECORD_STAND_INS + sm.OPEN_STAND_INS]  # (record-context; open-context)


@pytest.mark.gpu
@pytest.mark.parametrize("cls,name", LIVE, ids=[c.__name__ for c, _ in LIVE])
def test_the_comparisons_on_the_library_are_live(sfl, oracle, cls, name):
    """A model with a planted state fault, taken as the truth: the library does not have the fault, so some sequence of the
    subject (general; solid-context for the faults in the solids' state; viscous-context and viscous-batch for those in the
    viscosity's and the loads'; record-context and open-context for those in the recorders', the pivots', the averages' and the
    openings') must disagree -- in lazy or probing mode, as
    tests/test_sequences.py shows for models on both sides."""
    subject, seqs = sequences(name)
    hits = 0
    for case, ops in seqs.items():
        for mode in ("lazy", "probing"):
            model = cls(oracle, case[0], case[1], subject.batch) if subject.kind == "batch" else cls(oracle, case[0], case[1])
            model.viscous, model.records, model.opens, handle = subject.viscous, subject.records, subject.opens, subject.library(sfl, case)
            try:
                sm.replay(model, handle, ops, mode, seed=case[2])
            except AssertionError:
                hits += 1
            finally:
                handle.close()
    assert hits, f"{cls.__name__}: the library agreed with a faulty model in every sequence of {name}"
