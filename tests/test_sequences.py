"""The sequences of tests/sequence_model.py without a GPU: what the generator guarantees (a census computed from the op
lists alone), that the model computes the same bits with the oracle's port and with the compiled reference and stays
finite, and that the runner sees state bugs: three models with one planted fault each are caught by the sequences and
pass the kind of fresh-handle check the suite had before.  tests/test_sequences_gpu.py runs the same lists on the library.

The subjects with solids and histories (solid-context, solid-batch) have a census of their own: the planted walks -- a mask
set, replaced without a clear, cleared, with the fields left as they are -- every mask kind, every call that honours solids
under a mask with solid and fluid cells, masked solves of 0, 1 and 2 launches, the refusals where the generator planted them
and nowhere else, and three more faulty models that only a walk catches.  The op lists of the six subjects from before them
are pinned by digest: the new vocabulary must not move them.

The subjects with viscosity and loads (viscous-context, viscous-batch) have theirs: every launch class of the diffusion with a
reader of the velocity behind it, a viscosity in force while masks come and go, every plain path right behind a clear, the
companions of a viscous step, a batch's coefficients staged call after call, the loads' state (labels and masks in either order,
replaced and reset, a recorder across calls, restarted, sampling without a mask), the new refusals, planted and nowhere else --
all read from the op lists -- and, evaluated on the model, that no sequence compares only empty loads or diffusions that change
nothing.  Five more faulty models are caught by these sequences and missed by a fresh handle that makes each new call once.
The op lists of solid-context and solid-batch are pinned as they were before this vocabulary."""
import copy
import functools
import hashlib

import numpy as np
import pytest

import load_rule
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


# ... and the two subjects with solids and histories, as they were before the viscosity's and the loads' vocabulary was added
PINNED_SOLIDS = {"solid-context": "bca90f5609b44f816b9c9b7e93268830bb59800d34cb65c037ba4929641d6e18",
                 "solid-batch": "0606b2b680529158695b8c4aefa1b6deec695510de826aad615873ced9f4ad2e"}


@pytest.mark.parametrize("name", sorted(PINNED_SOLIDS))
def test_the_sequences_from_before_viscosity_and_loads_have_not_moved(name):
    subject, seqs = sequences(name)
    assert subject.solids and not subject.viscous and subject.length == 36
    assert hashlib.sha256(repr([seqs[case] for case in subject.cases]).encode()).hexdigest() == PINNED_SOLIDS[name]


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
SOLID_IDS = [s.name for s in sm.SUBJECTS if s.solids and not s.viscous]
VISCOUS_IDS = [s.name for s in sm.SUBJECTS if s.viscous]
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


@pytest.mark.parametrize("name", SOLID_IDS + VISCOUS_IDS)
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


# ---- viscosity and loads ---------------------------------------------------------------------------------------------------
READS_THE_VELOCITY = ("advect_velocity", "step", "calculate_divergence", "advance_tracers")
VISCOUS_REFUSALS = {"viscous-context": {("set_bodies", "recorder"), ("step_n", "full")},
                    "viscous-batch": {("set_bodies", "recorder"), ("step_n", "full"), ("step_n_until", "viscosity")}}


def viscous_walks(name):
    """[(case, [(index, op, what the Gate knows while the op runs, the path state, refused)])]: read from the op lists alone."""
    subject, seqs = sequences(name)
    out = []
    for case, ops in seqs.items():
        walk = []
        for (k, op, gate, refused), (_, _, path) in zip(sm.gated(ops, subject, case), sm.path_states(ops)):
            st = {"set": gate.masks is not None, "mixed": gate.mixed(), "hist": None if gate.hist is None else list(gate.hist), "trail": gate.trail,
                  "rec": gate.rec, "visc": None if gate.visc is None else dict(gate.visc), "labels": gate.labels,
                  "loads": None if gate.loads is None else list(gate.loads), "two_launches": gate.two_launches}
            walk.append((k, op, st, path, refused))
        out.append((case, walk))
    return subject, out


def due(recorder, op):
    """The samples the step call completes of a recorder [every, capacity, steps]."""
    every, _, steps = recorder
    return (steps + op[1].get("n", 1)) // every - steps // every


def in_force(st):
    """Whether a step call diffuses: a viscosity set, sweeps > 0 and some nu > 0."""
    return st["visc"] is not None and st["visc"]["sweeps"] > 0 and any(nu > 0 for nu in st["visc"]["nu"])


def test_the_two_viscous_subjects_and_their_shapes():
    by_name = {s.name: s for s in sm.SUBJECTS}
    assert [c for c in by_name["viscous-context"].cases] == sm._cases(130, 70, 3, 900) + sm._cases(61, 81, 2, 950)
    assert [c for c in by_name["viscous-batch"].cases] == sm._cases(61, 81, 3, 1000) + sm._cases(7, 9, 2, 1050) and by_name["viscous-batch"].batch == 3
    new = set(sm.VISCOUS_WRITERS + sm.VISCOUS_QUERIES)
    for name in VISCOUS_IDS:
        s = by_name[name]
        assert s.solids and not s.large and 40 <= s.length <= 50
        assert set(sm.SOLID_WRITERS + sm.SOLID_QUERIES) <= set(s.kinds())
        assert new - set(s.kinds()) == (set() if s.kind == "context" else {"diffuse_velocity"})
    assert not any(new & set(s.kinds()) for s in sm.SUBJECTS if not s.viscous), "no older subject's deck has a new kind"
    assert set(sm.LABEL_KINDS) == {"all one", "halves", "with zeros", "sixteen"}


def test_the_labels_cover_the_whole_grid_and_a_load_record_of_the_model_is_the_packages(sfl):
    assert load_rule.DTYPE == sfl.BODY_LOAD_DTYPE and sm.LOAD_BYTES == 48
    assert sm.body_labels("all one", 7, 9, 0) is None
    halves, zeros, sixteen = (sm.body_labels(kind, 130, 70, 4) for kind in ("halves", "with zeros", "sixteen"))
    assert halves.shape == (70, 130) and set(np.unique(halves)) == {1, 2} and (halves[:, :65] == 1).all() and (halves[:, 65:] == 2).all()
    assert set(np.unique(zeros)) == {0, 1, 2, 3} and 0.25 < (zeros == 0).mean() < 0.42
    assert set(np.unique(sixteen)) == set(range(1, 17)) and sixteen[3, 5] == 1 + 8
    for kind, bodies in sm.LABEL_KINDS.items():
        lab = sm.body_labels(kind, 7, 9, 1, member=2)
        assert lab is None or (lab.dtype == np.uint8 and int(lab.max()) <= bodies)


def test_census_every_launch_class_of_the_diffusion_hands_the_velocity_to_a_reader():
    subject, cases = viscous_walks("viscous-context")
    seen, again = set(), False
    for case, walk in cases:
        for k, (kind, a), st, _path, refused in walk[:-1]:
            launches = sm.launches_of(a["nu"], a["sweeps"]) if kind == "diffuse_velocity" else 0
            behind, later = walk[k + 1], walk[k + 2:]
            if launches and not refused and behind[1][0] in READS_THE_VELOCITY and not behind[4] and \
                    any(op[0] == "step_n" and op[1]["n"] >= 2 and not r for _, op, _, _, r in later):
                seen.add((case[:2], a["sweeps"]))
                again |= launches == 2 and st["two_launches"] >= 1
    for shape in ((130, 70), (61, 81)):
        assert {(shape, sweeps) for sweeps in (1, 9, 17)} <= seen, (shape, seen)
    assert again, "a two-launch diffusion on a handle that has made one before: the third buffer holds an old velocity"


def test_census_a_viscosity_is_in_force_while_masks_come_and_go():
    subject, cases = viscous_walks("viscous-context")
    seen = set()
    for case, walk in cases:
        set_behind = cleared_under = False          # a mask set / cleared since the viscosity was set
        for k, (kind, a), st, _path, refused in walk:
            if refused:
                continue
            if kind in ("set_viscosity", "clear_viscosity"):
                set_behind = cleared_under = False
            if kind == "set_solids" and in_force(st):
                set_behind, cleared_under = True, False
            if kind == "clear_solids" and in_force(st) and st["set"]:
                set_behind, cleared_under = False, True
            if kind in ("step", "step_n") and in_force(st):
                seen |= {(kind, "no mask")} if not st["set"] else set()
                seen |= {(kind, "a mixed mask")} if st["mixed"] else set()
                seen |= {(kind, "a mask set behind the viscosity")} if st["mixed"] and set_behind else set()
                seen |= {(kind, "the mask cleared while the viscosity stays")} if not st["set"] and cleared_under else set()
                seen.add((kind, f"{sm.launches_of(max(st['visc']['nu']), st['visc']['sweeps'])} launches"))
    for kind in ("step", "step_n"):
        for what in ("no mask", "a mixed mask", "a mask set behind the viscosity", "the mask cleared while the viscosity stays", "1 launches", "2 launches"):
            assert (kind, what) in seen, (kind, what, seen)


def test_census_a_cleared_viscosity_gives_every_plain_path_back():
    subject, cases = viscous_walks("viscous-context")
    seen = set()
    for case, walk in cases:
        for k, op, st, path, refused in walk[1:]:
            before = walk[k - 1]
            if before[1][0] != "clear_viscosity" or not in_force(before[2]) or op[0] not in ("step", "step_n") or refused:
                continue                                # (the step call right behind the clear of a viscosity that was in force)
            if case[:2] == (130, 70) and not st["set"] and st["hist"] is None and sm.takes_the_seam(op, path) and path["options"]["OPT_ADVECT_KERNEL"] == 2:
                seen.add("the step seams")
            if case[:2] == (61, 81) and not st["set"] and op[0] == "step" and sm.on_small_grid(path):
                seen.add("the one-launch step of a small grid")
            if not st["set"] and path["options"]["OPT_FUSE_PROJECTION"] == 0:
                seen.add("OPT_FUSE_PROJECTION = 0")
            if st["mixed"]:
                seen.add("a mask still set")
    assert seen == {"the step seams", "the one-launch step of a small grid", "OPT_FUSE_PROJECTION = 0", "a mask still set"}, seen


def test_census_a_viscous_step_has_every_companion():
    subject, cases = viscous_walks("viscous-context")
    seen = set()
    for case, walk in cases:
        for k, op, st, path, refused in walk:
            if op[0] in ("step", "step_n") and in_force(st) and not refused:
                hist, trail, loads = st["hist"] is not None and due(st["hist"], op) > 0, path["follow"] and st["trail"], st["loads"] is not None and due(st["loads"], op) > 0
                seen |= {name for name, on in (("history", hist), ("trail", trail), ("loads", loads)) if on}
                if hist and trail and loads and st["mixed"]:
                    seen.add("all three under a mixed mask")
                if hist and st["mixed"]:
                    seen.add("a history's sample under a viscosity and a mask")
    assert seen == {"history", "trail", "loads", "all three under a mixed mask", "a history's sample under a viscosity and a mask"}, seen


def test_census_a_batch_stages_its_coefficients_call_after_call():
    subject, cases = viscous_walks("viscous-batch")
    runs, seen = [], set()
    for case, walk in cases:
        run = []
        for k, op, st, path, refused in walk:
            kind, a = op
            mixed_nu = st["visc"] is not None and st["visc"]["per_member"] and st["visc"]["sweeps"] > 0 and 0.0 in st["visc"]["nu"] and max(st["visc"]["nu"]) > 0
            if kind in ("step_n", "step_n_each") and not refused and mixed_nu:
                run.append((kind, st["set"]))
            else:
                runs.append(run)
                run = []
            if kind == "set_viscosity" and not a["per_member"] and st["visc"] is not None and st["visc"]["per_member"]:
                seen.add("a per-member nu replaced by a shared one")
            cleared = st["visc"] is None and any(op2[0] == "clear_viscosity" for _, op2, _, _, _ in walk[:k])
            if cleared and kind == "step_n_until" and not refused:
                seen.add("cleared: step_n_until is taken")
            if cleared and kind == "step_n" and a["n"] >= 2 and not st["set"] and not path["follow"] and any(1 <= s < a["n"] for s in path["pending"]) and not refused:
                seen.add("cleared: the one-launch replay")
                if st["loads"] is not None and due(st["loads"], op) > 0:
                    seen.add("a loads sample inside the one-launch replay")
            if kind == "step_n_until" and refused and st["visc"] is not None and not st["set"]:
                assert walk[k + 1][1][0] in sm.STEPS and not walk[k + 1][4]
                seen.add("step_n_until refused for the viscosity alone")
            if kind in sm.STEPS and not refused and in_force(st):
                seen |= {"history"} if st["hist"] is not None and due(st["hist"], op) > 0 else set()
                seen |= {"frames"} if st["rec"] else set()
                seen |= {"following tracers"} if path["follow"] else set()
                seen |= {"loads under a mask"} if st["loads"] is not None and due(st["loads"], op) > 0 and st["mixed"] else set()
        runs.append(run)
    long = [r for r in runs if len(r) >= 3 and {k for k, _ in r} == {"step_n", "step_n_each"}]
    assert any(not any(m for _, m in r) for r in long), "three step calls in a row, both kinds, a per-member nu with a member at 0, no mask"
    assert any(all(m for _, m in r) for r in long), "... and under a mask"
    assert seen == {"a per-member nu replaced by a shared one", "cleared: step_n_until is taken", "cleared: the one-launch replay",
                    "a loads sample inside the one-launch replay", "step_n_until refused for the viscosity alone", "history", "frames", "following tracers",
                    "loads under a mask"}, seen


@pytest.mark.parametrize("name", VISCOUS_IDS)
def test_census_the_loads_state_is_walked(name):
    subject, cases = viscous_walks(name)
    seqs = sequences(name)[1]
    seen = set()
    for case, walk in cases:
        early, calls = False, None          # labels set while no mask is held; [step calls, a remainder left] of the recorder that is on
        for k, op, st, path, refused in walk:
            kind, a = op
            if refused:
                continue
            if kind == "set_bodies":
                early = a["label_kind"] != "all one" and not st["set"]
                seen |= {"labels replaced"} if st["labels"] is not None and a["label_kind"] != "all one" else set()
            if kind == "clear_bodies":
                early = False
                seen |= {"labels reset"} if st["labels"] is not None else set()
            if kind == "set_solids" and st["labels"] is not None:
                seen |= {"a mask replaced under labels"} if st["set"] else set()
            if kind == "clear_solids" and st["labels"] is not None and st["set"]:
                seen.add("a mask cleared under labels")
            if kind == "loads" and early and st["mixed"]:
                seen.add("labels set before the mask")
            if kind == "loads_start":
                calls = [0, False]
                seen |= {"a restart while on"} if st["loads"] is not None else set()
            if kind == "loads_stop":
                calls = None
            if kind in sm.STEPS and st["loads"] is not None:
                every, _, steps = st["loads"]
                calls[0] += 1
                calls[1] |= (steps + a.get("n", 1)) % every != 0
                if every in (2, 3) and calls[0] >= 3 and calls[1]:
                    seen.add("a recorder across three calls that leave a remainder")
                seen.add(f"counted through {kind}")
                if due(st["loads"], op) > 0 and not st["set"]:
                    seen.add("a sample while no mask is set")
                    if subject.kind == "context" and sm.takes_the_seam(op, path) and st["hist"] is None and case[:2] == (130, 70) and path["options"]["OPT_ADVECT_KERNEL"] == 2:
                        seen.add("a sample inside the seam loop")
    want = {"labels set before the mask", "a mask replaced under labels", "a mask cleared under labels", "labels replaced", "labels reset", "a restart while on",
            "a recorder across three calls that leave a remainder", "a sample while no mask is set"}
    want |= {"a sample inside the seam loop", "counted through step", "counted through step_n"} if subject.kind == "context" else \
            {"counted through step_n", "counted through step_n_each", "counted through step_n_until"}
    assert seen == want, (name, want - seen, seen - want)


@pytest.mark.parametrize("name", VISCOUS_IDS)
def test_census_the_new_refusals_are_the_planted_ones(name):
    subject, cases = viscous_walks(name)
    causes = set()
    for case, walk in cases:
        for k, (kind, a), st, path, refused in walk:
            if not refused:
                continue
            if kind in ("set_bodies", "clear_bodies"):
                assert st["loads"] is not None and walk[k + 1][1][0] in sm.STEPS and not walk[k + 1][4]
                causes.add((kind, "recorder"))
            elif kind == "step_n_until" and st["visc"] is not None and not st["set"]:
                causes.add((kind, "viscosity"))
            else:
                # the third admission check refuses: the loads recorder is full, the history and the trail (a batch: the frames) are not
                assert kind in sm.STEPS and st["loads"] is not None and due(st["loads"], (kind, a)) > st["loads"][1] - st["loads"][2] // st["loads"][0]
                assert st["hist"] is not None and due(st["hist"], (kind, a)) <= st["hist"][1] - st["hist"][2] // st["hist"][0]
                assert (path["follow"] and st["trail"]) if subject.kind == "context" else st["rec"]
                behind = [op[0] for _, op, _, _, _ in walk[k + 1:k + 6]]
                assert set(behind[:3]) == {"history", "trail" if subject.kind == "context" else "frames", "loads_history"}, behind
                assert behind[3] == "loads_stop" and behind[4] in sm.STEPS and not walk[k + 5][4], behind
                causes.add((kind, "full"))
    assert causes == VISCOUS_REFUSALS[name], (name, causes)
    assert sum(r for _, walk in cases for *_, r in walk) == len(VISCOUS_REFUSALS[name]), "only the planted refusals happen"


@pytest.mark.parametrize("name", VISCOUS_IDS)
def test_no_sequence_passes_vacuously(name, oracle):
    """Evaluated on the model: in every sequence a compared load has faces and a force, and a viscous step changes the velocity's
    bits against the same step with the viscosity taken away."""
    subject, seqs = sequences(name)
    for case, ops in seqs.items():
        model = subject.model(oracle, case)
        loaded = diffused = False
        for op in ops:
            kind = op[0]
            twin = None
            members = model.m if subject.kind == "batch" else [model]
            if kind in sm.STEPS and any(m.visc is not None and m.visc[0] > 0 and m.visc[1] > 0 for m in members) and not model.refuses(*op):
                twin = copy.deepcopy(model, {id(oracle): oracle})
                for m in (twin.m if subject.kind == "batch" else [twin]):
                    m.visc = None
            out = model.apply(op)
            if twin is not None:
                twin.apply(op)
                a, b = model.snapshot()["velocity"], twin.snapshot()["velocity"]
                diffused |= a.tobytes() != b.tobytes()
            if kind in ("loads", "loads_history") and "records" in out and out["records"].size:
                rec = np.ascontiguousarray(out["records"]).view(load_rule.DTYPE).reshape(-1)
                loaded |= bool(((rec["faces"].sum(axis=-1) > 0) & ((rec["fx"] != 0) | (rec["fy"] != 0))).any())
        assert loaded, (name, case, "no compared load has faces and a force")
        assert diffused, (name, case, "no viscous step changes the velocity")


def make_stand_in(cls, oracle):
    return lambda s, c: cls(oracle, c[0], c[1], s.batch) if s.kind == "batch" else cls(oracle, c[0], c[1])


@pytest.mark.parametrize("cls", sm.VISCOUS_STAND_INS + sm.LOAD_STAND_INS, ids=[c.__name__ for c in sm.VISCOUS_STAND_INS + sm.LOAD_STAND_INS])
def test_a_planted_viscosity_or_loads_bug_is_caught_by_the_sequences_and_missed_by_a_fresh_handle(cls, oracle):
    subject, seqs = sequences(sm.stand_in_subject(cls))
    hits = []
    for case, ops in seqs.items():
        for mode in ("lazy", "probing"):
            try:
                sm.run(subject, case, ops, mode, oracle, make_stand_in(cls, oracle))
            except AssertionError as e:
                hits.append((case, mode, str(e).splitlines()[0]))
    print(cls.__name__, hits)
    assert hits, f"{cls.__name__}: no sequence of {subject.name} saw the fault"
    assert all("seed" in h[2] and "mode" in h[2] and "op " in h[2] for h in hits), "a failure names seed, mode and op"
    if subject.kind == "batch":         # every new call once on a fresh handle, one order: nothing seen
        sm.viscous_batch_fresh_handle_check(oracle, lambda dim_x, dim_y: cls(oracle, dim_x, dim_y, 3))
    else:
        sm.viscous_fresh_handle_check(oracle, lambda dim_x, dim_y: cls(oracle, dim_x, dim_y))
        solid_fresh_handle_check(oracle, lambda dim_x, dim_y: cls(oracle, dim_x, dim_y))
        sm.fresh_handle_check(oracle, lambda dim_x, dim_y: cls(oracle, dim_x, dim_y))
