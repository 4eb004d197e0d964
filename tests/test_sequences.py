"""The sequences of tests/sequence_model.py without a GPU: what the generator guarantees (a census computed from the op
lists alone), that the model computes the same bits with the oracle's port and with the compiled reference and stays
finite, and that the runner sees state bugs: three models with one planted fault each are caught by the sequences and
pass the kind of fresh-handle check the suite had before.  tests/test_sequences_gpu.py runs the same lists on the library.

The subjects with solids and histories (solid-context, solid-batch) have a census of their own: the planted walks -- a mask
set, replaced without a clear, cleared, with the fields left as they are -- every mask kind, every call that honours solids
under a mask with solid and fluid cells, masked solves of 0, 1 and 2 launches, the refusals where the generator planted them
and nowhere else, and three more faulty models that only a walk catches.  The op lists of the six subjects from before them
are pinned by digest: the new vocabulary must not move them."""
import functools
import hashlib

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


# SHA-256 over repr of generate()'s op lists, case by case, as they were before the solids' vocabulary was added
PINNED = {"general": "6dd52e312f48d14a15a0e11441522a7107308356e41e3e426122fcc87cf71773",
          "seams": "ae83840075cb710ffe46b63a2d7cae07386fa6620b8b6de569f9c9b7527c634a",
          "one-workgroup": "38ab1b15959df2eae73ab9c989d295509b383fd5678b7d5e6f62b4611a8cbeb8",
          "slabs": "2140deadce65835b4ff81cb2d1757257094bd6da66eb8d7bf56a1f54c9bc5479",
          "small-batch": "8acb6d31c872bca80650f49e9717a7d11bf06d1f588d331a50787a2f01bf2335",
          "large-batch": "c88947597a38cd09d9b62c3da0c57e7ea3aac80c3cc9d0d572edc58366112603"}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_the_sequences_from_before_solids_have_not_moved(name):
    subject, seqs = sequences(name)
    assert not subject.solids and subject.length == 30
    assert hashlib.sha256(repr([seqs[case] for case in subject.cases]).encode()).hexdigest() == PINNED[name]


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


# ---- solids and histories ------------------------------------------------------------------------------------------------
SOLID_IDS = [s.name for s in sm.SUBJECTS if s.solids]
HONOURED = {"context": ("step", "step_n", "calculate_divergence", "poisson_solve", "poisson_continue", "subtract_gradient", "residual",
                        "poisson_solve_until", "flow_stats"),
            "batch": ("step_n", "step_n_each", "poisson_solve", "poisson_solve_each", "flow_stats")}
PLANTED_REFUSALS = {"solid-context": 3, "solid-batch": 8}


def walks(name):
    """[(case, [(index, op, a copy of what the Gate knows while the op runs, refused)])] of a subject with solids."""
    subject, seqs = sequences(name)
    out = []
    for case, ops in seqs.items():
        walk = []
        for k, op, gate, refused in sm.gated(ops, subject, case):
            state = {"set": gate.masks is not None, "mixed": gate.mixed(), "masks": gate.masks, "per_member": gate.masks is not None and len(gate.masks) > 1,
                     "hist": None if gate.hist is None else list(gate.hist), "rec": gate.rec, "view": gate.view}
            walk.append((k, op, state, refused))
        out.append((case, walk))
    return subject, out


def test_the_two_subjects_and_their_shapes():
    by_name = {s.name: s for s in sm.SUBJECTS}
    assert [c[:2] for c in by_name["solid-context"].cases] == [(130, 70)] * 3 + [(61, 81)] * 2
    assert [c[:2] for c in by_name["solid-batch"].cases] == [(61, 81)] * 3 + [(7, 9)] * 2 and by_name["solid-batch"].batch == 3
    assert all(by_name[n].length == 36 and not by_name[n].large for n in SOLID_IDS)
    for name in SOLID_IDS:
        assert set(sm.SOLID_WRITERS + sm.SOLID_QUERIES) <= set(by_name[name].kinds())
    assert not any(set(sm.SOLID_WRITERS + sm.SOLID_QUERIES) & set(s.kinds()) for s in sm.SUBJECTS if not s.solids)


def test_a_history_record_of_the_model_has_every_field_of_the_packages(sfl):
    assert set(sm.HISTORY_FIELDS) == set(sfl.HISTORY_DTYPE.names)
    for name, dtype in sm.HISTORY_FIELDS.items():
        assert sfl.HISTORY_DTYPE[name].base == np.dtype(dtype), name
    assert sm.ERR_STATE == sfl.capi.ERR_STATE and sm.VIEW_DIVERGENCE == sfl.capi.VIEW_DIVERGENCE


@pytest.mark.parametrize("name", SOLID_IDS)
def test_census_masks_and_the_calls_that_honour_them(name):
    subject, cases = walks(name)
    steps = [(case, walk) for case, walk in cases]
    set_kinds, stepped_under, honoured, launches, replaced = set(), set(), set(), set(), 0
    for case, walk in steps:
        under = None                                    # the kind of the mask in force, until a step call has run under it
        for k, (kind, a), st, refused in walk:
            if refused:
                continue
            if kind == "set_solids":
                set_kinds.add(a["mask_kind"])
                replaced += st["set"]
                under = a["mask_kind"]
            elif kind == "clear_solids":
                under = None
            elif kind in sm.STEPS and under is not None:
                stepped_under.add(under)
            if st["mixed"]:
                honoured.add(kind)
                if kind in sm.STEPS and st["hist"] is not None and (st["hist"][2] + a.get("n", 1)) // st["hist"][0] > st["hist"][2] // st["hist"][0]:
                    honoured.add("a history's sample")
                if subject.kind == "context" and kind in ("poisson_solve", "poisson_continue", "step", "step_n"):
                    launches.add(-(-a["iters"] // sm.D_SOLID))
    assert set_kinds == set(sm.MASK_KINDS), (name, set_kinds)
    assert stepped_under == set(sm.MASK_KINDS), (name, "every mask kind in front of a step call", stepped_under)
    assert set(HONOURED[subject.kind]) <= honoured, (name, set(HONOURED[subject.kind]) - honoured)
    assert replaced >= 2, "a mask set over a mask"
    if subject.kind == "context":
        assert "a history's sample" in honoured and launches == {0, 1, 2}, (honoured, launches)
    else:
        shared = {st["per_member"] for _, walk in steps for _, (kind, _a), st, r in walk if st["set"] and kind in sm.STEPS and not r}
        assert shared == {False, True}, "a shared mask and one per member, both stepped under"
        drawn = {st["view"] for _, walk in steps for _, (kind, _a), st, r in walk if st["mixed"] and st["rec"] and kind in sm.STEPS and not r}
        assert None in drawn and drawn & {0, 1, 2}, ("the recorder draws the dye and a view next to a mask", drawn)
        assert any(kind == "envelope" and st["mixed"] for _, walk in steps for _, (kind, _a), st, _ in walk)


@pytest.mark.parametrize("name", SOLID_IDS)
def test_census_refusals_are_the_planted_ones_and_a_step_call_follows_each(name):
    subject, cases = walks(name)
    total = 0
    for case, walk in cases:
        refused = [k for k, _, _, r in walk if r]
        total += len(refused)
        assert len(refused) <= 4, (name, case, "at most 4 of 36 ops are refused", refused)
        for k in refused:
            assert walk[k + 1][1][0] in sm.STEPS and not walk[k + 1][3], (name, case, k, walk[k][1], "a step call the header takes follows")
        masked = [k for k, (kind, _a), st, r in walk if st["mixed"] and not r and kind not in sm.QUERIES and kind != "set_option"]
        assert len(masked) >= 10, (name, case, "writers under a mask with solid and fluid cells", len(masked))
    assert total == PLANTED_REFUSALS[name], (name, total)
    causes = {(kind, "full" if kind in sm.STEPS and not (st["set"] and kind == "step_n_until") else "solids" if st["set"] else "history or view")
              for _, walk in cases for _, (kind, _a), st, r in walk if r}
    want = ({("view_scalar", "solids"), ("view_texels", "solids"), ("step_n", "full")} if subject.kind == "context" else
            {("step_n_until", "solids"), ("poisson_solve_until", "solids"), ("history_start", "solids"), ("record_view", "solids"),
             ("view_render_members", "solids"), ("set_solids", "history or view"), ("step_n", "full")})
    assert causes == want, (name, causes)
    if subject.kind == "batch":     # set_solids refused for both of its reasons
        why = {("history" if st["hist"] is not None else "view") for _, walk in cases for _, (kind, _a), st, r in walk if r and kind == "set_solids"}
        assert why == {"history", "view"}, why


def test_census_a_cleared_context_takes_its_plain_paths_again_and_options_have_their_say_under_a_mask():
    subject, cases = walks("solid-context")
    seqs = sequences("solid-context")[1]
    seam = small = False
    in_force = set()
    for case, walk in cases:
        cleared = False
        for (k, op, st, refused), (_, _, path) in zip(walk, sm.path_states(seqs[case])):
            cleared |= op[0] == "clear_solids"
            plain = cleared and not st["set"] and not refused
            if plain and case[:2] == (130, 70) and st["hist"] is None and sm.takes_the_seam(op, path) and path["options"]["OPT_ADVECT_KERNEL"] == 2:
                seam = True
            if plain and case[:2] == (61, 81) and op[0] == "step" and sm.on_small_grid(path):
                small = True
            if st["set"] and not refused:
                in_force |= {(option, value) for option, value in path["options"].items() if op[0] in sm.AFFECTS[option]}
    assert seam, "cleared at 130 x 70: a step_n that takes the step seams"
    assert small, "cleared at 61 x 81: the one-launch step of a small grid"
    for option, values in subject.option_values().items():
        for value in values:
            assert (option, value) in in_force, ("in force while a mask is set, in front of a writer it would otherwise affect", option, value)


@pytest.mark.parametrize("name", SOLID_IDS)
def test_census_a_queued_record_lies_on_a_solid_cell_and_one_on_a_fluid_cell_of_the_mask_set_behind_it(name):
    subject, seqs = sequences(name)
    chain = [c for what, c in sm.handovers_of(subject).items() if what.startswith("queue_forces(step = 2) -> set_solids")][0]
    hits = 0
    for case, ops in seqs.items():
        for at in range(len(ops) - len(chain) + 1):
            if sm.has_handover(ops[at:at + len(chain)], chain):
                (_, q), (_, m) = ops[at], ops[at + 1]
                mask = sm.solid_mask(m["mask_kind"], case[0], case[1], m["seed"])
                on = [bool(mask[j, i]) for i, j in q["cells"]]
                assert True in on and False in on, (name, case, q, on)
                hits += 1
    assert hits


@pytest.mark.parametrize("name", SOLID_IDS)
def test_the_model_refuses_what_the_census_says_is_refused(name, oracle):
    """The models decide from the fields and counts they hold, the census from the op list: the same ops, and a refused op
    changes nothing in the model."""
    subject, cases = walks(name)
    seqs = sequences(name)[1]
    for case, walk in cases:
        model = subject.model(oracle, case)
        for (k, op, _, refused) in walk:
            before = model.snapshot()
            got = model.apply(op)
            assert (isinstance(got, dict) and "refused" in got) == refused, (name, case, k, op)
            if refused:
                assert got["refused"] == sm.ERR_STATE
                sm.compare(model.snapshot(), before, "a refused op")


def solid_fresh_handle_check(oracle, make_handle, dim_x=61, dim_y=81, seed=3):
    """The kind of check the direct tests of the solids are: a fresh handle, one mask, one fixed order -- steps, the operators
    one by one, a continued solve of D + 1 iterations (two launches) over an uploaded pressure, the norm and the statistics;
    then cleared ONCE, every field uploaded again, one step."""
    up = lambda field: ("upload", {"field": field, "texture_kind": "noise", "seed": seed})
    solve = {"dx": 0.5, "iters": 5, "omega": 1.5}
    step = ("step", dict({"dt": 1 / 30.0}, **solve))
    ops = [up(sm.FV), up(sm.FC), ("set_solids", {"mask_kind": "disc", "seed": 7}), ("solids", {}), ("step_n", dict({"n": 3, "dt": 1 / 30.0}, **solve)),
           ("calculate_divergence", {"dx": 0.5}), ("poisson_solve", solve), ("residual", {"dx": 0.5}), up(sm.FP),
           ("poisson_continue", dict(solve, iters=sm.D_SOLID + 1)), ("download", {"field": sm.FP}), ("residual", {"dx": 0.5}), ("subtract_gradient", {"dx": 0.5}),
           ("flow_stats", {"dx": 0.5}), ("history_start", {"every": 1, "capacity": 4}), step, ("history", {}), ("history_stop", {}),
           ("clear_solids", {}), up(sm.FV), up(sm.FC), up(sm.FD), up(sm.FP), step]
    model, handle = sm.ContextModel(oracle, dim_x, dim_y), make_handle(dim_x, dim_y)
    for op in ops:
        want, got = model.apply(op), handle.apply(op)
        if want is not None:
            sm.compare(got, want, f"a fresh handle, one order: {op[0]}")
    sm.compare(handle.snapshot(), model.snapshot(), "a fresh handle, one order")


@pytest.mark.parametrize("cls", sm.SOLID_STAND_INS, ids=[c.__name__ for c in sm.SOLID_STAND_INS])
def test_a_planted_solids_bug_is_caught_by_the_sequences_and_missed_by_a_fresh_handle(cls, oracle):
    subject, seqs = sequences("solid-context")
    hits = caught(subject, seqs, oracle, cls, ("lazy", "probing"))
    print(cls.__name__, hits)
    assert hits, f"{cls.__name__}: no sequence of solid-context saw the fault"
    solid_fresh_handle_check(oracle, lambda dim_x, dim_y: cls(oracle, dim_x, dim_y))     # one mask, one order, one clear: nothing seen
    sm.fresh_handle_check(oracle, lambda dim_x, dim_y: cls(oracle, dim_x, dim_y))
