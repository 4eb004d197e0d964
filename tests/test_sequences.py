"""The sequences of tests/sequence_model.py without a GPU: what the generator guarantees (a census computed from the op
lists alone), that the model computes the same bits with the oracle's port and with the compiled reference and stays
finite, and that the runner sees state bugs: three models with one planted fault each are caught by the sequences and
pass the kind of fresh-handle check the suite had before.  tests/test_sequences_gpu.py runs the same lists on the library."""
import functools

import numpy as np
import pytest

import sequence_model as sm
from oracle import loader

IDS = [s.name for s in sm.SUBJECTS]


@functools.lru_cache(maxsize=None)
def sequences(name):
    subject = next(s for s in sm.SUBJECTS if s.name == name)
    return subject, sm.generate(subject, loader.port())


@pytest.mark.parametrize("name", IDS)
def test_the_generator_is_deterministic_and_prints_literals(name):
    subject, seqs = sequences(name)
    again = sm.generate(subject, loader.port())
    assert repr(again) == repr(seqs)
    for ops in seqs.values():
        assert len(ops) == subject.length
        assert eval(repr(ops), {"inf": np.inf, "nan": np.nan}) == ops, "an op list is a Python literal"


@pytest.mark.parametrize("name", IDS)
def test_census_kinds_options_and_textures(name):
    subject, seqs = sequences(name)
    ops = [op for seq in seqs.values() for op in seq]
    count = {}
    for kind, _ in ops:
        count[kind] = count.get(kind, 0) + 1
    print(name, sorted(count.items()))
    assert set(count) <= set(subject.kinds()), "only calls include/sfl.h permits for the subject"
    for kind in subject.kinds():
        assert count.get(kind, 0) >= 3, (name, kind, count.get(kind, 0))
    set_values = {(a["name"], a["value"]) for kind, a in ops if kind == "set_option"}
    for option, values in subject.option_values().items():
        for value in values:
            assert (option, value) in set_values, (name, option, value)
    uploaded = {a["texture_kind"] for kind, a in ops if kind == "upload" and a["field"] == sm.FV}
    assert uploaded == set(sm.TEXTURES), (name, uploaded)
    dye = [sm.texture("noise", sm.FC, 9, 7, seed) for seed in range(3)]
    assert max(int(c.max()) for c in dye) >= 2 ** 31 and max(int(c.max()) for c in dye) < 0xFF000000, "dye reaches the upper half of UQ32"
    for kind, a in ops:      # the parameter ranges
        for key, allowed in (("dt", sm.DTS), ("dx", sm.DXS), ("omega", sm.OMEGAS)):
            for x in (a[key] if isinstance(a.get(key), list) else [a[key]] if key in a else []):
                assert x in allowed, (kind, key, x)
        for x in (a["iters"] if isinstance(a.get("iters"), list) else [a["iters"]] if "iters" in a else []):
            assert 0 <= x <= sm.MAX_ITERS
        assert a.get("n", 1) <= 4


@pytest.mark.parametrize("name", IDS)
def test_census_hand_overs(name):
    subject, seqs = sequences(name)
    for what, chain in sm.handovers_of(subject).items():
        assert any(sm.has_handover(ops, chain) for ops in seqs.values()), (name, what)


@pytest.mark.parametrize("name", IDS)
def test_census_every_option_value_is_in_force_while_a_call_it_affects_runs(name):
    subject, seqs = sequences(name)
    seen = set()
    for ops in seqs.values():
        for _, (kind, _a), state in sm.path_states(ops):
            seen |= {(option, value) for option, value in state["options"].items() if kind in sm.AFFECTS[option]}
    for option, values in subject.option_values().items():
        if sm.option_applies(subject, option):
            for value in values:
                assert (option, value) in seen, (name, option, value)


def test_census_the_paths_each_subject_is_there_for():
    """The option block and the follow flag are followed through every op list: the calls below run while the path is taken."""
    states = lambda name: [(case, list(sm.path_states(ops)), ops) for case, ops in sequences(name)[1].items()]
    # the general kernels at 130 x 70: the tiled advection family needs OPT_ADVECT_KERNEL = 2 there (9100 cells: auto is untiled)
    tiled = {kind for _, walk, _ in states("general") for _, (kind, _a), st in walk if st["options"]["OPT_ADVECT_KERNEL"] == 2}
    assert {"step", "advect_velocity", "advect_color", "calculate_divergence", "subtract_gradient"} <= tiled, tiled
    untiled = {kind for _, walk, _ in states("general") for _, (kind, _a), st in walk if st["options"]["OPT_ADVECT_KERNEL"] == 1}
    assert "advect_velocity" in untiled
    # the fused step boundary on exact sources: both lattice textures, no solve, dt = 0.25, every condition of the seam
    for texture in ("landing", "whole-cell"):
        assert any(sm.takes_the_seam(op, st) and st["lattice"] == texture and op[1]["iters"] == 0 and op[1]["dt"] == 0.25
                   for _, walk, _ in states("seams") for _, op, st in walk), texture
    assert all(any(sm.takes_the_seam(op, st) for _, op, st in walk) for _, walk, _ in states("seams")), "a seam in every sequence"
    # one workgroup, the general kernels and back, a solve or a step after each flip, on one handle
    def flips(walk):
        path = [sm.on_small_grid(st) for _, (kind, _a), st in walk if kind in sm.SOLVES]
        runs = [p for k, p in enumerate(path) if k == 0 or p != path[k - 1]]
        return any(runs[k:k + 3] == [True, False, True] for k in range(len(runs)))
    assert any(flips(walk) for case, walk, _ in states("one-workgroup") if case[:2] == (61, 81))
    assert any(flips(walk) for case, walk, _ in states("one-workgroup") if case[:2] == (2, 2))
    # slabs: the velocity flips by upload on a handle that has stepped, and a step follows at once; under both halos
    for texture in ("noise", "fast", "still"):
        assert any(kind == "upload" and a["field"] == sm.FV and a["texture_kind"] == texture and st["stepped"] and ops[k + 1][0] == "step"
                   for _, walk, ops in states("slabs") for k, (kind, a), st in walk if k + 1 < len(ops)), texture
    fixed = {kind for _, walk, _ in states("slabs") for _, (kind, _a), st in walk if st["options"]["OPT_ADVECT_HALO"] == sm.FIXED_HALO}
    assert {"step", "advect_velocity", "advect_color"} <= fixed, fixed


@pytest.mark.parametrize("name", IDS)
def test_census_writers_run_all_along_a_sequence(name):
    """No long run of reads and option changes: in every window of 8 ops something writes a field, the timeline or the tracers."""
    subject, seqs = sequences(name)
    for case, ops in seqs.items():
        quiet = [kind in sm.QUERIES or kind == "set_option" for kind, _ in ops]
        for at in range(len(ops) - 7):
            assert not all(quiet[at:at + 8]), (name, case, at, [k for k, _ in ops[at:at + 8]])


def test_lattice_textures_stay_on_the_lattice(oracle):
    """What the landing and whole-cell textures are for: at dt = 0.25 a whole-cell velocity keeps multiples of 4 over four
    steps without a solve (so every source is a cell centre), and both textures give finite fields."""
    m = sm.ContextModel(oracle, 61, 45)
    m.apply(("upload", {"field": sm.FV, "texture_kind": "whole-cell", "seed": 1}))
    m.apply(("upload", {"field": sm.FC, "texture_kind": "whole-cell", "seed": 1}))
    m.apply(("step_n", {"n": 4, "dt": 0.25, "dx": 1.0, "iters": 0, "omega": 1.0}))
    assert np.array_equal(m.v, np.round(m.v / 4) * 4) and np.count_nonzero(m.v) > m.v.size // 5
    m.apply(("upload", {"field": sm.FV, "texture_kind": "landing", "seed": 2}))
    m.apply(("step_n", {"n": 2, "dt": 0.25, "dx": 1.0, "iters": 3, "omega": 1.96}))
    assert m.finite()


class Quiet:
    """A model standing in for the handle."""

    def __init__(self, cls):
        self.cls = cls

    def __call__(self, subject, case):
        return self.cls(loader.port(), case[0], case[1]) if subject.kind != "batch" else self.cls(loader.port(), case[0], case[1], subject.batch)


@pytest.mark.parametrize("name", IDS)
def test_the_model_is_finite_and_agrees_with_itself_in_every_mode(name, oracle):
    """Every sequence through the model, a second model as the handle: every field after every op is finite, every query of
    the probing mode is answerable, and the three modes hold."""
    subject, seqs = sequences(name)
    handle = Quiet(type(subject.model(oracle, subject.cases[0])))
    for case, ops in seqs.items():
        sm.run(subject, case, ops, "probing", oracle, handle, check_finite=True)
    case = subject.cases[-1]
    for mode in ("eager", "lazy"):
        sm.run(subject, case, seqs[case], mode, oracle, handle)


@pytest.mark.parametrize("name", IDS)
def test_the_model_gives_the_same_bits_with_the_port_and_the_reference(name, oracle, reference):
    subject, seqs = sequences(name)
    for case, ops in seqs.items():
        a, b = subject.model(oracle, case), subject.model(reference, case)
        sm.replay(a, b, ops, "eager", seed=case[2], label=f"{name}: port against reference")


def caught(subject, seqs, oracle, cls, modes):
    hits = []
    for case, ops in seqs.items():
        for mode in modes:
            try:
                sm.run(subject, case, ops, mode, oracle, lambda s, c: cls(oracle, c[0], c[1]))
            except AssertionError as e:
                hits.append((case, mode, str(e).splitlines()[0]))
    return hits


@pytest.mark.parametrize("cls", sm.STAND_INS, ids=[c.__name__ for c in sm.STAND_INS])
@pytest.mark.parametrize("name", ["general"])
def test_a_planted_state_bug_is_caught_by_the_sequences_and_missed_by_a_fresh_handle(name, cls, oracle):
    subject, seqs = sequences(name)
    hits = caught(subject, seqs, oracle, cls, ("lazy", "probing"))
    print(cls.__name__, hits)
    assert hits, f"{cls.__name__}: no sequence of {name} saw the fault"
    assert all("seed" in h[2] and "mode" in h[2] and "op " in h[2] for h in hits), "a failure names seed, mode and op"
    sm.fresh_handle_check(oracle, lambda dim_x, dim_y: cls(oracle, dim_x, dim_y))      # the old kind of check sees nothing
    with pytest.raises(AssertionError):                                               # (and the runner's message replays)
        case, mode, _ = hits[0]
        sm.run(subject, case, seqs[case], mode, oracle, lambda s, c: cls(oracle, c[0], c[1]))


def test_a_failure_message_carries_what_replay_needs(oracle):
    subject, seqs = sequences("general")
    with pytest.raises(AssertionError) as e:
        for case, ops in seqs.items():
            sm.run(subject, case, ops, "probing", oracle, lambda s, c: sm.TimelineStaysAfterStepN(oracle, c[0], c[1]))
    text = str(e.value)
    assert "seed" in text and "mode probing" in text and "replay(model, handle, ops, 'probing'" in text
    literal = text.split("with ops =\n", 1)[1]
    ops = eval(literal, {"inf": np.inf})
    assert isinstance(ops, list) and ops and ops == seqs[case][:len(ops)]
