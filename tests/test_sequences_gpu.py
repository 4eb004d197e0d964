"""The call sequences of tests/sequence_model.py on the library: one live handle per sequence -- a whole-domain context on
the general kernels, with the fused step boundaries and on the one-workgroup path, a group of three virtual ranks, a
small and a large batch -- taken through 30 seeded ops and compared with the model bit for bit, in three modes over the
same op list: every field after every op (eager), nothing read before the end (lazy), one seeded query after every op
(probing).  tests/test_sequences.py has the census of what the lists contain.

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


@pytest.mark.gpu
@pytest.mark.parametrize("cls", sm.STAND_INS, ids=[c.__name__ for c in sm.STAND_INS])
def test_the_comparisons_on_the_library_are_live(sfl, oracle, cls):
    """A model with a planted state fault, taken as the truth: the library does not have the fault, so some sequence of the
    general subject must disagree -- in lazy or probing mode, as tests/test_sequences.py shows for models on both sides."""
    subject, seqs = sequences("general")
    hits = 0
    for case, ops in seqs.items():
        for mode in ("lazy", "probing"):
            model, handle = cls(oracle, case[0], case[1]), subject.library(sfl, case)
            try:
                sm.replay(model, handle, ops, mode, seed=case[2])
            except AssertionError:
                hits += 1
            finally:
                handle.close()
    assert hits, f"{cls.__name__}: the library agreed with a faulty model in every sequence"
