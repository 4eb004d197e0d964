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
The op lists of solid-context and solid-batch are pinned as they were before this vocabulary.

Four more subjects walk the features that came after: record-context and record-batch the friction and the torque recorder, the
pivots and the averages on top of the viscous vocabulary, open-context and open-batch the openings, the inflow profiles and the
flux on top of the solids'.  Their census reads every planted chain and every refusal -- with its code -- from the op lists;
the vacuity conditions are evaluated on the model; ten more faulty models are caught by these sequences and missed by a fresh
handle.  The op lists of viscous-context and viscous-batch are pinned as they were before."""
import copy
import functools
import hashlib

import numpy as np
import pytest

import friction_rule
import inflow_rule
import load_rule
import mean_rule
import opening_rule
import sequence_model as sm
import torque_rule
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


# ... and the two with viscosity and loads, as they were before the openings', the friction's, the torque's and the averages'
PINNED_VISCOUS = {"viscous-context": "93ef1888e616857f3e7ce146876eadc52db13c104f8db6b0bbe3bd47e27e4240",
                  "viscous-batch": "b655f2643b07acfba0b73fd585cca85636d7c247fb786a68c862f208cd0722bf"}


@pytest.mark.parametrize("name", sorted(PINNED_VISCOUS))
def test_the_sequences_from_before_openings_and_recorders_have_not_moved(name):
    subject, seqs = sequences(name)
    assert subject.viscous and not subject.records and not subject.opens and subject.length == sm.VISCOUS_LENGTH[subject.kind]
    assert hashlib.sha256(repr([seqs[case] for case in subject.cases]).encode()).hexdigest() == PINNED_VISCOUS[name]


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
SOLID_IDS = [s.name for s in sm.SUBJECTS if s.solids and not s.viscous and not s.opens]
VISCOUS_IDS = [s.name for s in sm.SUBJECTS if s.viscous and not s.records]
RECORD_IDS = [s.name for s in sm.SUBJECTS if s.records]
OPEN_IDS = [s.name for s in sm.SUBJECTS if s.opens]
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
                     "hist": None if gate.hist is None else list(gate.hist), "rec": gate.rec, "view": gate.view,
                     "code": gate.code(*op) if refused else None}
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


@pytest.mark.parametrize("name", SOLID_IDS + VISCOUS_IDS + RECORD_IDS + OPEN_IDS)
def test_the_model_refuses_what_the_census_says_is_refused(name, oracle):
    """The models decide from the fields and counts they hold, the census from the op list: the same ops, the same code, and a
    refused op changes nothing in the model."""
    subject, cases = walks(name)
    seqs = sequences(name)[1]
    for case, walk in cases:
        model = subject.model(oracle, case)
        for (k, op, st, refused) in walk:
            before = model.snapshot()
            got = model.apply(op)
            assert (isinstance(got, dict) and "refused" in got) == refused, (name, case, k, op)
            if refused:
                assert got["refused"] == st["code"] and (st["code"] == sm.ERR_STATE or name in RECORD_IDS + OPEN_IDS)
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
    assert not any(new & set(s.kinds()) for s in sm.SUBJECTS if not s.viscous and not s.opens), "no older subject's deck has a new kind"
    for s in sm.SUBJECTS:       # (the subjects with openings, which came later, take the two calls that plant their refusals and no other)
        if s.opens:
            assert new & set(s.kinds()) == {"set_viscosity", "clear_viscosity"}
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


def records_of(out, dtype):
    """The records a query returned as raw bytes, as a flat array of the struct."""
    return np.ascontiguousarray(out["records" if "records" in out else "record"]).reshape(-1).view(dtype)


@pytest.mark.parametrize("name", VISCOUS_IDS + RECORD_IDS + OPEN_IDS)
def test_no_sequence_passes_vacuously(name, oracle):
    """Evaluated on the model: in every sequence a compared load has faces and a force, and a viscous step changes the velocity's
    bits against the same step with the viscosity taken away.  In every sequence with the three recorders a compared friction
    record has a force, a compared torque record has both moments about a pivot that is not (0, 0), and a plane of at least two
    samples is downloaded under a mask; in every sequence with openings a step runs under a map with a live inflow and a live
    outflow cell, a compared flux record has both sums, and a step runs under a profile that differs from the uniform inflow on
    a live cell.  (check_finite of the model's own run covers that the fields stay finite.)"""
    subject, seqs = sequences(name)
    for case, ops in seqs.items():
        model = subject.model(oracle, case)
        loaded = diffused = False
        seen = set()
        for op in ops:
            kind = op[0]
            twin = None
            members = model.m if subject.kind == "batch" else [model]
            if kind in sm.STEPS and not model.refuses(*op):
                for m in members:
                    if m.open is not None and all(sm.live_cells(m.open, m.mask)):
                        seen.add("a step under a live inflow and a live outflow cell")
                    fluid_inflow = opening_rule.inflow_cells(m.open, m.mask) if m.open is not None else None
                    if m.profile and any(fluid_inflow[j, i] and tuple(np.float32(uv)) != tuple(np.float32(m.inflow)) for (i, j), uv in inflow_rule.unique(m.profile)):
                        seen.add("a step under a profile that differs from the uniform inflow on a live cell")
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
            if not isinstance(out, dict) or "refused" in out:
                continue
            if kind in ("friction", "friction_history") and out["records"].size:
                rec = records_of(out, friction_rule.DTYPE)
                seen |= {"a friction record with a force"} if ((rec["fx"] != 0) | (rec["fy"] != 0)).any() else set()
            if kind in ("torque", "torque_history") and out["records"].size:
                rec = records_of(out, torque_rule.DTYPE)
                seen |= {"a torque record with both moments about a pivot"} if ((rec["mp"] != 0) & (rec["mf"] != 0) & (rec["pivot2"] != 0).any(axis=-1)).any() else set()
            if kind == "mean_sums" and model.means["samples"] >= 2 and any(sm.mixed(m.mask) for m in members):
                seen.add("a plane of two samples under a mask")
            if kind == "openings_flux":
                rec = records_of(out, inflow_rule.FLUX_DTYPE)
                seen |= {"a flux record with both sums"} if ((rec["inflow"] != 0) & (rec["outflow"] != 0)).any() else set()
        if name in VISCOUS_IDS:
            assert loaded, (name, case, "no compared load has faces and a force")
            assert diffused, (name, case, "no viscous step changes the velocity")
        want = {"a friction record with a force", "a torque record with both moments about a pivot", "a plane of two samples under a mask"} if name in RECORD_IDS else \
               {"a step under a live inflow and a live outflow cell", "a flux record with both sums",
                "a step under a profile that differs from the uniform inflow on a live cell"} if name in OPEN_IDS else set()
        assert want <= seen, (name, case, want - seen)


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


# ---- friction, torque and averages; openings, profiles and the flux ---------------------------------------------------------
def later_walks(name):
    """[(case, [(index, op, what the Gate knows while the op runs, the path state, refused)])] of the four later subjects."""
    subject, seqs = sequences(name)
    out = []
    for case, ops in seqs.items():
        walk = []
        for (k, op, gate, refused), (_, _, path) in zip(sm.gated(ops, subject, case), sm.path_states(ops)):
            st = {"set": gate.masks is not None, "mixed": gate.mixed(), "masks": gate.masks, "hist": None if gate.hist is None else list(gate.hist), "trail": gate.trail,
                  "rec": gate.rec, "view": gate.view, "visc": None if gate.visc is None else dict(gate.visc), "labels": gate.labels,
                  "loads": None if gate.loads is None else list(gate.loads), "friction": None if gate.friction is None else list(gate.friction),
                  "torque": None if gate.torque is None else list(gate.torque), "means": None if gate.means is None else dict(gate.means),
                  "ranges": dict(gate.ranges), "bodies": gate.bodies, "pivots": gate.pivots, "open": gate.open, "inflow": gate.inflow, "profile": gate.profile,
                  "live": gate.live(), "code": gate.code(*op) if refused else None}
            walk.append((k, op, st, path, refused))
        out.append((case, walk))
    return subject, out


def has_room(recorder, op):
    every, capacity, steps = recorder
    return due(recorder, op) <= capacity - steps // every


def fused(subject, case, op, st, path):
    """The step call that runs fused when nothing cuts it: a context's step_n over its seams on the seam shape (every condition
    set), a batch's one-launch replay of a timeline (a record in a later step of the call, no following set)."""
    if st["set"] or st["visc"] is not None or st["hist"] is not None or st["open"] is not None:
        return False
    if subject.kind == "context":
        return case[:2] == (130, 70) and sm.takes_the_seam(op, path) and path["options"]["OPT_ADVECT_KERNEL"] == 2
    return op[0] == "step_n" and op[1]["n"] >= 2 and not path["follow"] and any(1 <= s < op[1]["n"] for s in path["pending"])


def test_the_four_later_subjects_and_their_shapes():
    by_name = {s.name: s for s in sm.SUBJECTS}
    for new, old in (("record-context", "viscous-context"), ("record-batch", "viscous-batch"), ("open-context", "solid-context"), ("open-batch", "solid-batch")):
        a, b = by_name[new], by_name[old]
        assert [c[:2] for c in a.cases] == [c[:2] for c in b.cases] and a.batch == b.batch and a.kind == b.kind and not a.large
        assert set(b.kinds()) <= set(a.kinds()), "on top of the older deck"
    for name in RECORD_IDS:
        assert set(by_name[name].kinds()) - set(by_name[name.replace("record", "viscous")].kinds()) == set(sm.RECORD_WRITERS + sm.RECORD_QUERIES)
        assert by_name[name].length == sm.RECORD_LENGTH[by_name[name].kind]
    for name in OPEN_IDS:
        assert set(by_name[name].kinds()) - set(by_name[name.replace("open", "solid")].kinds()) == set(sm.OPEN_WRITERS + sm.OPEN_QUERIES)
        assert by_name[name].length == sm.OPEN_LENGTH[by_name[name].kind]
    new = set(sm.RECORD_WRITERS + sm.RECORD_QUERIES + sm.OPEN_WRITERS + sm.OPEN_QUERIES) - {"set_viscosity", "clear_viscosity"}
    assert not any(new & set(s.kinds()) for s in sm.SUBJECTS if not (s.records or s.opens)), "no older subject's deck has a new kind"
    for s in sm.SUBJECTS[-4:]:      # the shortest the deck fits in: one op less and the planner has no room
        shorter = copy.copy(s)
        shorter.length = s.length - 1
        with pytest.raises(AssertionError, match="does not fit"):
            sm.plan(shorter)


def test_the_records_and_the_maps_of_the_model_are_the_packages(sfl):
    assert friction_rule.DTYPE == sfl.BODY_FRICTION_DTYPE and friction_rule.DTYPE.itemsize == 48
    assert torque_rule.DTYPE == sfl.BODY_TORQUE_DTYPE and torque_rule.DTYPE.itemsize == 64
    assert inflow_rule.FLUX_DTYPE == sfl.OPEN_FLUX_DTYPE and sm.FLUX_BYTES == 40
    assert sm.ERR_INVALID == sfl.capi.ERR_INVALID and sfl.capi.MEAN_ALL == mean_rule.ALL == 15
    for kind in sm.OPEN_KINDS:
        for member in (None, 0, 2):
            for shape in ((130, 70), (61, 81), (7, 9)):
                m = sm.open_map(kind, *shape, 3, member)
                assert m.dtype == np.uint8 and m.shape == shape[::-1] and opening_rule.check_map(m) is None
    count = lambda kind: sm.live_cells(sm.open_map(kind, 61, 81, 3), None)
    assert count("channel") == (79, 79) and count("inflow only") == (79, 0) and count("outflow only") == (0, 79 + 59) and count("none") == (0, 0)
    assert count("single inflow") == (1, 0) and sum(count("every rim cell")) == 2 * (79 + 59) and min(count("every rim cell")) > 0
    assert all(min(sm.live_cells(sm.open_map(kind, 7, 9, seed, member), None)) > 0 for kind in sm.LIVE_OPEN_KINDS for seed in range(4) for member in (None,))
    for kind in sm.PIVOT_KINDS:
        p = sm.body_pivots_of(kind, 16, 61, 81, 5, member=1)
        assert p.dtype == np.int32 and p.shape == (16, 2) and (p != 0).any(axis=1).all() and np.abs(p).max() <= torque_rule.MAX_PIVOT2


def test_float64_planes_are_compared_as_their_bit_patterns():
    a = np.array([[0.0, np.nan, 1.5]])
    sm.compare({"plane": a.copy()}, {"plane": a}, "a NaN equals itself")
    for other in (np.array([[-0.0, np.nan, 1.5]]), np.array([[0.0, -np.nan, 1.5]]), np.array([[0.0, np.nan, np.nextafter(1.5, 2)]])):
        with pytest.raises(AssertionError, match="differ bitwise"):
            sm.compare({"plane": other}, {"plane": a}, "+0.0 is not -0.0, a NaN of another sign is another NaN, one ulp is a difference")
    with pytest.raises(AssertionError):
        sm.compare({"plane": a.astype(np.float32)}, {"plane": a}, "no cast on either side")


@pytest.mark.parametrize("name", RECORD_IDS)
def test_census_the_recorders_the_pivots_and_the_averages_are_walked(name):
    subject, cases = later_walks(name)
    batch, seen, whats = subject.kind == "batch", set(), set()
    for case, walk in cases:
        five = 0                        # step calls in a row with all five counters on
        sampled = None                  # the pivots under which the torque recorder that is on has taken a sample
        zero_run = []                   # every == 0: fused call, mean_sample, fused call, mean_sample
        for k, op, st, path, refused in walk:
            kind, a = op
            behind = walk[k + 1] if k + 1 < len(walk) else None
            on = {n: st[n] for n in ("hist", "loads", "friction", "torque") if st[n] is not None}
            averaging = st["means"] is not None and st["means"]["every"] >= 1
            if kind == "mean_start" and not refused:
                whats.add(a["what"])
                if st["means"] is not None and st["means"]["samples"] > 0:
                    seen.add("the averages restarted while on, behind a sample")
            if kind in ("friction_start", "torque_start") and st[kind[:-len("_start")]] is not None and st[kind[:-len("_start")]][2] > 0:
                seen.add(f"{kind}: a restart while on")
            if kind in sm.STEPS and not refused:
                if len(on) == 4 and averaging:
                    everys = {r[0] for r in on.values()} | {st["means"]["every"]}
                    five = five + 1 if len(everys) == 5 else 0
                    if five >= 3 and any((r[2] + a.get("n", 1)) % r[0] for r in on.values()):
                        seen.add("all five counters on, five periods, three calls, remainders")
                    if batch and len({st["ranges"][n] for n in ("loads", "friction", "torque", "mean")}) == 4:
                        seen.add("the ranges of the recorders differ")
                else:
                    five = 0
                for n in ("friction", "torque"):
                    if st[n] is not None:
                        seen.add(f"{n}: counted through {kind}")
                        if due(st[n], op) > 0 and in_force(st) and st["mixed"]:
                            seen.add(f"{n}: a sample behind a viscous step under a mask")
                if averaging:
                    seen.add(f"averages: counted through {kind}")
                    m, n = st["means"], a.get("n", 1)
                    if fused(subject, case, op, st, path) and any((m["steps"] + j) % m["every"] == 0 for j in range(1, n)):
                        seen.add("averages with every >= 1: a sample due inside a call that would run fused")
                if st["torque"] is not None and due(st["torque"], op) > 0 and st["mixed"]:
                    now = ("none", 0) if st["pivots"] is None else (st["pivots"]["pivot_kind"], st["pivots"]["seed"])
                    if sampled is not None and sampled != now:
                        seen.add("torque samples before and behind a change of the pivots while recording")
                    sampled = sampled or now
                if st["means"] is not None and st["means"]["every"] == 0 and fused(subject, case, op, st, path):
                    zero_run = zero_run + ["fused"] if zero_run[-1:] != ["fused"] else zero_run
            if kind in ("torque_start", "torque_stop"):
                sampled = None
            if kind == "mean_sample" and not refused and st["means"]["every"] == 0 and zero_run[-1:] == ["fused"]:
                zero_run.append("sample")
                if zero_run[-4:] == ["fused", "sample", "fused", "sample"]:
                    seen.add("averages with every == 0: mean_sample between fused calls")
            if kind in ("mean_start", "mean_stop"):
                zero_run = []
            if kind == "mean_stop" and averaging and behind is not None and fused(subject, case, behind[1], behind[2], behind[3]) and not behind[4]:
                seen.add("mean_stop, then the fused path again")
            if kind in ("set_solids", "clear_solids") and not refused and st["set"] and st["friction"] and st["torque"] and averaging and behind[1][0] in sm.STEPS:
                seen.add(f"{kind} under a mask while the three record, a step behind it")
            if kind == "set_bodies" and not refused and st["pivots"] is not None:
                same = sm.LABEL_KINDS[a["label_kind"]] == st["bodies"]
                asked = any(op2[0] == "body_pivots" for _, op2, *_ in walk[k + 1:k + 3])
                seen |= {"set_bodies to the same number with pivots set" if same else "set_bodies to another number with pivots set"} if asked else set()
            if kind == "set_bodies" and not refused and st["pivots"] is None and st["bodies"] != sm.LABEL_KINDS[a["label_kind"]] and \
                    any(o2[0] == "set_body_pivots" and o2[1]["pivot_kind"] and o2[1]["bodies"] == sm.LABEL_KINDS[a["label_kind"]] and not r2 for _, o2, _, _, r2 in walk[:k]) and \
                    walk[k + 1][1][0] == "body_pivots":
                seen.add("set_bodies back to a number whose pivots were put back to zero, the pivots read behind it")
            if kind == "clear_bodies" and not refused and st["pivots"] is not None and st["bodies"] != 1:
                seen.add("clear_bodies with pivots set")
            if kind == "set_body_pivots" and not refused and a["pivot_kind"] is None and st["pivots"] is not None:
                seen.add("set_body_pivots(NULL) over pivots")
            if refused:
                assert behind[1][0] in sm.STEPS and not behind[4], (name, case, k, op, "a step call the header takes follows")
                if kind in ("set_bodies", "clear_bodies"):
                    assert st["loads"] is None and len(on) - (st["hist"] is not None) == 1
                    seen.add(f"{kind}, refused under the {'friction' if st['friction'] else 'torque'} recorder alone")
                elif kind in sm.STEPS:
                    full = [n for n, r in on.items() if not has_room(r, op)]
                    assert len(on) == 4 and averaging and len(full) == 1 and full[0] in ("friction", "torque"), (name, case, k, full)
                    assert behind[1][1].get("n", 1) == 2, "the call behind it fits: two samples, the capacity"
                    asked = {op2[0] for _, op2, *_ in walk[k + 2:k + 8]}
                    assert {"history", "loads_history", "friction_history", "torque_history", "mean_info"} <= asked, "every count is read behind it"
                    seen.add(f"a full {full[0]} recorder refuses the call whole while the others have room")
                elif kind == "set_body_pivots":
                    assert st["code"] == sm.ERR_INVALID and a["bodies"] != st["bodies"] and st["pivots"] is not None
                    assert any(op2[0] == "body_pivots" for _, op2, *_ in walk[k + 2:k + 4])
                    seen.add("set_body_pivots with another number of bodies, refused")
                else:
                    assert kind == "mean_sums" and st["code"] == sm.ERR_INVALID and not st["means"]["what"] & mean_rule.GROUP_OF[a["plane"]]
                    seen.add("a plane outside what, refused")
    want = {"the averages restarted while on, behind a sample", "friction_start: a restart while on", "torque_start: a restart while on",
            "all five counters on, five periods, three calls, remainders", "friction: a sample behind a viscous step under a mask",
            "torque: a sample behind a viscous step under a mask", "averages with every >= 1: a sample due inside a call that would run fused",
            "torque samples before and behind a change of the pivots while recording", "averages with every == 0: mean_sample between fused calls",
            "mean_stop, then the fused path again", "set_solids under a mask while the three record, a step behind it",
            "clear_solids under a mask while the three record, a step behind it", "set_bodies to the same number with pivots set",
            "set_bodies to another number with pivots set", "clear_bodies with pivots set",
            "set_bodies back to a number whose pivots were put back to zero, the pivots read behind it", "set_body_pivots(NULL) over pivots",
            "a full friction recorder refuses the call whole while the others have room", "a full torque recorder refuses the call whole while the others have room",
            "set_body_pivots with another number of bodies, refused", "a plane outside what, refused"}
    want |= {f"{kind}, refused under the {n} recorder alone" for kind in ("set_bodies", "clear_bodies") for n in ("friction", "torque")}
    steps = ("step_n", "step_n_each") if batch else ("step", "step_n")
    want |= {f"{n}: counted through {kind}" for n in ("friction", "torque", "averages") for kind in steps}
    want |= {"the ranges of the recorders differ", "averages: counted through step_n_until"} if batch else set()
    assert want <= seen, (name, want - seen)
    assert sum(r for _, walk in cases for *_, r in walk) == 8, "only the planted refusals happen"
    groups = lambda w: bin(w).count("1")
    assert {min(groups(w), 2) for w in whats if w != 15} == {1, 2} and 15 in whats, ("what masks of one group, of several and of all", whats)


LATER_STAND_INS = sm.RECORD_STAND_INS + sm.OPEN_STAND_INS


@pytest.mark.parametrize("cls", LATER_STAND_INS, ids=[c.__name__ for c in LATER_STAND_INS])
def test_a_planted_recorder_or_openings_bug_is_caught_by_the_sequences_and_missed_by_a_fresh_handle(cls, oracle):
    subject, seqs = sequences(sm.later_stand_in_subject(cls))
    hits = caught(subject, seqs, oracle, cls, ("lazy", "probing"))
    print(cls.__name__, hits)
    assert hits, f"{cls.__name__}: no sequence of {subject.name} saw the fault"
    assert all("seed" in h[2] and "mode" in h[2] and "op " in h[2] for h in hits), "a failure names seed, mode and op"
    make = lambda dim_x, dim_y: cls(oracle, dim_x, dim_y)       # every new call once on a fresh handle, one order: nothing seen
    sm.record_fresh_handle_check(oracle, make)
    sm.open_fresh_handle_check(oracle, make)
    sm.viscous_fresh_handle_check(oracle, make)
    solid_fresh_handle_check(oracle, make)
    sm.fresh_handle_check(oracle, make)


def test_a_map_with_no_opening_gives_the_solids_bits_and_with_no_solid_cell_the_plain_step(oracle):
    """The anchor of "OPENINGS" on the model: the same ops with and without a map that has no opening, under a mask and without."""
    up = lambda field: ("upload", {"field": field, "texture_kind": "noise", "seed": 5})
    step = ("step_n", {"n": 2, "dt": 0.1, "dx": 0.5, "iters": 9, "omega": 1.96})
    for mask in (("set_solids", {"mask_kind": "seeded", "seed": 2}), ("clear_solids", {})):
        a, b = sm.ContextModel(oracle, 33, 18), sm.ContextModel(oracle, 33, 18)
        for op in (up(sm.FV), up(sm.FC), mask):
            a.apply(op), b.apply(op)
        a.apply(("set_openings", {"open_kind": "none", "seed": 0, "inflow": [12.5, 0.0]}))
        for op in (step, ("calculate_divergence", {"dx": 3.0}), ("poisson_solve", {"dx": 3.0, "iters": 5, "omega": 1.5}), ("subtract_gradient", {"dx": 3.0})):
            a.apply(op), b.apply(op)
            sm.compare(a.snapshot(), b.snapshot(), f"{mask[0]}, no opening: {op[0]}")
        for q in (("residual", {"dx": 0.5}), ("flow_stats", {"dx": 0.5})):
            sm.compare(a.apply(q), b.apply(q), f"{mask[0]}, no opening: {q[0]}")


OPEN_REFUSALS = {
    "open-context": {("set_openings", "viscosity"), ("view_scalar", "openings"), ("view_texels", "openings"), ("set_viscosity", "openings"),
                     ("set_inflow", "no openings"), ("set_inflow_profile", "no openings"), ("set_inflow_profile", "off the inflow cells")},
    "open-batch": {("set_openings", "history"), ("set_openings", "view"), ("set_openings", "viscosity"), ("step_n_until", "openings"),
                   ("poisson_solve_until", "openings"), ("history_start", "openings"), ("record_view", "openings"), ("view_render_members", "openings"),
                   ("set_viscosity", "openings"), ("set_inflow", "no openings"), ("set_inflow_profile", "no openings"),
                   ("set_inflow_profile", "off the inflow cells")},
}


def applies_to(profile, member):
    """The cells of a set_inflow_profile's records that go to `member`."""
    return [tuple(c) for k, c in enumerate(profile["cells"]) if profile.get("members") is None or profile["members"][k] == member]


@pytest.mark.parametrize("name", OPEN_IDS)
def test_census_the_openings_the_profiles_and_the_refusals_are_walked(name):
    subject, cases = later_walks(name)
    batch, members, seen, causes, stepped_under = subject.kind == "batch", range(max(subject.batch, 1)), set(), set(), set()
    for case, walk in cases:
        first = None                    # which of the map and the mask, both held, was set first
        under = None                    # the kind of the map in force, until a step call has run under it
        gone = None                     # an inflow cell with a profile record that a mask made solid: what has been seen since, by phase
        for k, op, st, path, refused in walk:
            kind, a = op
            behind = walk[k + 1] if k + 1 < len(walk) else None
            is_open, live = st["open"] is not None, st["live"]
            if refused:
                assert behind[1][0] in sm.STEPS and not behind[4], (name, case, k, op, "a step call the header takes follows")
                assert st["code"] == (sm.ERR_INVALID if kind == "set_inflow_profile" and is_open else sm.ERR_STATE)
                if kind == "set_openings":
                    why = [n for n, on in (("history", batch and st["hist"] is not None), ("view", batch and st["rec"] and st["view"] == sm.VIEW_DIVERGENCE),
                                           ("viscosity", st["visc"] is not None)) if on]
                    assert len(why) == 1
                    causes.add((kind, why[0]))
                elif kind in ("set_inflow", "set_inflow_profile") and not is_open:
                    causes.add((kind, "no openings"))
                elif kind == "set_inflow_profile":
                    assert st["profile"] is not None and any(op2[0] == "inflow_profile" for _, op2, *_ in walk[k + 2:k + 4]), "the profile as it was is read behind it"
                    causes.add((kind, "off the inflow cells"))
                else:
                    assert is_open and not st["set"] or kind in ("view_scalar", "view_texels", "record_view", "view_render_members", "set_viscosity") and is_open
                    causes.add((kind, "openings"))
                continue
            if kind == "set_openings":
                first = "mask" if st["set"] else "map"
                under = a["open_kind"]
                if st["profile"] is not None and behind[1][0] == "inflow_profile":
                    seen.add("a new map under a profile, the profile read behind it")
            if kind == "clear_openings":
                first, under = ("mask" if st["set"] else None), None
            if kind == "set_solids" and not st["set"]:
                first = "map" if is_open else "mask"
            if kind == "clear_solids":
                first = "map" if is_open else None
            if kind in sm.STEPS:
                if is_open and st["set"] and first is not None:
                    seen.add(f"a step under a map and a mask, the {first} set first")
                if under is not None:
                    stepped_under.add(under)
                if is_open and batch:
                    seen.add(f"{kind} under {'per-member' if len(st['open']) > 1 else 'shared'} maps and {'per-member' if len(st['inflow']) > 1 else 'shared'} inflows")
                if is_open and min(live) > 0:
                    seen |= {"a history's sample under a map"} if st["hist"] is not None and due(st["hist"], op) > 0 else set()
                    seen |= {"a trail and a following set under a map"} if path["follow"] and st["trail"] else set()
                    seen |= {"following tracers under a map"} if path["follow"] else set()
            if kind in ("set_solids", "clear_solids") and is_open and st["set"] and behind[1][0] in sm.STEPS:
                seen.add(f"{kind} over a mask behind a map, a step right after")
            if kind == "set_inflow" and is_open and behind[1][0] in sm.STEPS and [tuple(u) for u in (a["inflow"] if a.get("per_member") else [a["inflow"]])] != st["inflow"]:
                seen.add(f"set_inflow {'with' if st['profile'] is not None else 'without'} a profile held, a step after")
            if kind == "set_inflow_profile" and is_open and behind[1][0] in sm.STEPS:
                if st["profile"] is not None:
                    seen.add("a profile replaced, a step after" if a["cells"] else "a profile cleared, a step after")
                for m in members:
                    cells = applies_to(a, m)
                    vels = [tuple(u) for k2, u in enumerate(a["vels"]) if a.get("members") is None or a["members"][k2] == m]
                    seen |= {"a profile with a duplicate cell"} if len(set(cells)) < len(cells) else set()
                    seen |= {"a profile with a record equal to the uniform inflow"} if tuple(st["inflow"][m if len(st["inflow"]) > 1 else 0]) in vels else set()
            if kind == "queue_forces" and is_open:
                for m, (i, j) in zip(a.get("members", [0] * len(a["cells"])), a["cells"]):
                    held = st["open"][m if len(st["open"]) > 1 else 0]
                    if 0 <= i < case[0] and 0 <= j < case[1] and held[j, i]:
                        on = "an outflow" if held[j, i] == opening_rule.OUTFLOW else "a profiled" if st["profile"] and (i, j) in applies_to(st["profile"], m) else "an inflow"
                        seen.add(f"a queued force record on {on} cell")
            if is_open and min(live) > 0 and kind in ("calculate_divergence", "poisson_solve", "poisson_continue", "subtract_gradient", "poisson_solve_until", "residual",
                                                      "flow_stats", "poisson_solve_each"):
                seen.add(f"{kind} under a map")
            # an inflow cell with a profile record on it goes solid and comes back
            if kind == "set_solids" and is_open and st["profile"] is not None:
                solid = [sm.solid_mask(a["mask_kind"], case[0], case[1], a["seed"], m if a.get("per_member") else None) for m in members]
                named = [c for m in members for c in applies_to(st["profile"], m) if solid[m][c[1], c[0]]]
                gone = {"phase": "solid", "solid": set(), "back": set()} if named and behind[2]["live"][0] < live[0] else None
            elif gone is not None and kind in ("set_openings", "clear_openings", "set_inflow_profile", "set_solids"):
                gone = None
            elif gone is not None and kind == "clear_solids" and gone["phase"] == "solid":
                gone["phase"] = "back"
                assert behind[2]["live"][0] > live[0], "the live count comes back"
            elif gone is not None:
                gone[gone["phase"]].add("step" if kind in sm.STEPS else kind)
                if {"openings", "step", "openings_flux", "inflow_profile"} <= gone["solid"] and {"openings", "step", "openings_flux"} <= gone["back"]:
                    seen.add("an inflow cell with a profile record goes solid and comes back, the counts, the flux and the profile read in both states")
            # a cleared map gives the plain paths back: the step call right behind the clear
            if kind == "clear_openings" and is_open and behind is not None and not behind[4]:
                op2, st2, path2 = behind[1], behind[2], behind[3]
                if not batch:
                    seen |= {"cleared: the step seams"} if fused(subject, case, op2, st2, path2) else set()
                    seen |= {"cleared: the one-launch step of a small grid"} if case[:2] == (61, 81) and op2[0] == "step" and not st2["set"] and sm.on_small_grid(path2) else set()
                    seen |= {"cleared: the unfused step"} if op2[0] == "step" and not st2["set"] and path2["options"]["OPT_FUSE_PROJECTION"] == 0 else set()
                    seen |= {"cleared: step_n with the seams switched off"} if op2[0] == "step_n" and path2["options"]["OPT_STEP_SEAMS"] == 0 else set()
                    seen |= {"cleared with a mask still set"} if op2[0] in sm.STEPS and st2["mixed"] else set()
                else:
                    later = [(o[0], r) for _, o, _, _, r in walk[k + 1:k + 14]]
                    seen |= {"cleared: step_n_until"} if ("step_n_until", False) in later else set()
                    seen |= {"cleared: poisson_solve_until"} if ("poisson_solve_until", False) in later else set()
                    seen |= {"cleared: history_start"} if ("history_start", False) in later else set()
                    seen |= {"cleared: the one-launch replay"} if any(fused(subject, case, o, s, p) and not r for _, o, s, p, r in walk[k + 1:k + 14]) else set()
                    seen |= {"cleared with a mask still set"} if op2[0] in sm.STEPS and st2["mixed"] else set()
    want = {"a step under a map and a mask, the map set first", "a step under a map and a mask, the mask set first", "set_solids over a mask behind a map, a step right after",
            "clear_solids over a mask behind a map, a step right after", "set_inflow with a profile held, a step after", "set_inflow without a profile held, a step after",
            "a new map under a profile, the profile read behind it", "a profile replaced, a step after", "a profile cleared, a step after", "a profile with a duplicate cell",
            "a profile with a record equal to the uniform inflow", "a queued force record on an inflow cell", "a queued force record on a profiled cell",
            "a queued force record on an outflow cell", "an inflow cell with a profile record goes solid and comes back, the counts, the flux and the profile read in both states",
            "cleared with a mask still set"}
    if batch:
        want |= {f"{kind} under {maps} maps and {inflows} inflows" for kind, maps, inflows in (("step_n", "shared", "shared"), ("step_n_each", "per-member", "per-member"))}
        want |= {"poisson_solve_each under a map", "poisson_solve under a map", "flow_stats under a map", "cleared: step_n_until", "cleared: poisson_solve_until",
                 "cleared: history_start", "cleared: the one-launch replay", "following tracers under a map"}
    else:
        want |= {f"{kind} under a map" for kind in ("calculate_divergence", "poisson_solve", "poisson_continue", "subtract_gradient", "poisson_solve_until", "residual", "flow_stats")}
        want |= {"a history's sample under a map", "a trail and a following set under a map", "cleared: the step seams", "cleared: the one-launch step of a small grid",
                 "cleared: the unfused step", "cleared: step_n with the seams switched off"}
    assert want <= seen, (name, want - seen)
    assert stepped_under == set(sm.OPEN_KINDS), (name, "every kind of map in front of a step call", set(sm.OPEN_KINDS) - stepped_under)
    assert causes == OPEN_REFUSALS[name], (name, causes ^ OPEN_REFUSALS[name])
    assert sum(r for _, walk in cases for *_, r in walk) == len(OPEN_REFUSALS[name]), "only the planted refusals happen"
