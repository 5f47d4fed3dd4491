"""Buffer discipline of the two-lane denoise step and of the two engine slots, checked on the host (no GPU, no launch).

bench.py captures every CldmEngine.step_prog into a hipGraph whose two branches are the ControlNet (lane 1, its own arena) and the
UNet encoder + middle block (lane 0), and keeps two engine slots in flight on two streams.  Eager replay, which every other test
uses, runs the launch list in list order on one stream and cannot see a buffer that both branches or both slots touch.  The rules
below are read off the launch records (every device tensor a launch uses is in its ``keep``) of engines built on the CPU; the
captured forms themselves are run in tests/test_gpu_graphs.py."""
import pytest
import torch

from edtr_amd.testing import ranges_overlap, rec_ranges, tensor_range

ENGINES = [("fast", 2, 16, 16), ("fast", 1, 24, 16), ("fast", 16, 64, 64),      # (16, 64, 64): the halo tile takes the 32 x 32 level
           ("mixed", 2, 16, 16), ("high", 2, 16, 16), ("hybrid", 2, 16, 16)]

# What the two lanes may share between fork and join: launch name of the lane-1 reader -> why the memory is read-only there.
# Nothing today: the two networks have separate weights, and what the ControlNet reads of lane 0's arena is written before the fork.
LANES_MAY_SHARE = {}


def _union(recs):
    out = set()
    for r in recs:
        out |= rec_ranges(r)
    return out


def _inside(r, outer):
    return any(o[0] <= r[0] and r[1] <= o[1] for o in outer)


def _chunks(arena):
    return {tensor_range(c) for c in arena.chunks}


def _span(prog):
    fork = [i for i, m in prog.marks.items() if m == "fork"]
    join = [i for i, m in prog.marks.items() if m == "join"]
    assert len(fork) == 1 and len(join) == 1 and len(prog.marks) == 2, prog.marks
    assert fork[0] < join[0]
    return fork[0], join[0]


def _lane_recs(prog, lane):
    f, j = _span(prog)
    return [r for i, r in enumerate(prog.recs) if f <= i < j and prog.lanes[i] == lane]


def _lane_overlap(eng):
    """{range: names of the lane-1 launches that use it} for the lane-1 ranges that a lane-0 launch between fork and join touches."""
    one, zero = _lane_recs(eng.step_prog, 1), _lane_recs(eng.step_prog, 0)
    hit = ranges_overlap(_union(one), _union(zero))
    return {rg: sorted({r.name for r in one if rg in rec_ranges(r)}) for rg in hit}


def _build_engine(cldm, B, h, w):
    """(CldmEngine built outside the model's cache, the accumulator tensors Program.sums_slot handed to its step program)."""
    from edtr_amd.engine import Program
    from edtr_amd.model.cldm import CldmEngine
    handed = []
    real = Program.sums_slot

    def recording(self, arena, B, count=1):
        t = real(self, arena, B, count)
        handed.append((self, t))
        return t

    Program.sums_slot = recording
    try:
        eng = CldmEngine(cldm, B, h, w, 77)
    finally:
        Program.sums_slot = real
    return eng, [t for p, t in handed if p is eng.step_prog]


@pytest.fixture(scope="module")
def models():
    from edtr_amd import synth
    from edtr_amd.testing import build_synthetic_cldm
    made = {}

    def get(precision):
        if precision not in made:
            made[precision] = build_synthetic_cldm(synth.tiny_config(), "cpu", torch.bfloat16, precision=precision)
        return made[precision]
    return get


@pytest.fixture(scope="module")
def engines(models):
    made = {}

    def get(case):
        if case not in made:
            made[case] = _build_engine(models(case[0]), *case[1:])
        return made[case]
    return get


# ---------------------------------------------------------------------------------------------------------------------
# the checker itself
# ---------------------------------------------------------------------------------------------------------------------
def _rec(*keep):
    from edtr_amd.ops import Rec
    return Rec(None, (), keep, "hand-made")


def test_range_of_a_strided_view_runs_to_its_last_element():
    buf = torch.zeros(8, 16)
    left, right = buf[:, :8], buf[:, 8:]
    assert tensor_range(buf) == (buf.data_ptr(), buf.data_ptr() + 8 * 16 * 4)
    assert tensor_range(left) == (buf.data_ptr(), buf.data_ptr() + (7 * 16 + 7 + 1) * 4)
    assert tensor_range(right) == (buf.data_ptr() + 8 * 4, buf.data_ptr() + 8 * 16 * 4)
    assert tensor_range(buf[3]) == (buf.data_ptr() + 3 * 16 * 4, buf.data_ptr() + 4 * 16 * 4)


def test_two_column_slices_of_one_buffer_are_reported():
    buf = torch.zeros(8, 16, dtype=torch.bfloat16)
    a, b = _rec(object(), buf[:, :8]), _rec(buf[:, 8:], None)
    assert ranges_overlap(rec_ranges(a), rec_ranges(b)) == rec_ranges(a)
    assert ranges_overlap(rec_ranges(b), rec_ranges(a)) == rec_ranges(b)
    # ... rows of it are apart
    assert not ranges_overlap(rec_ranges(_rec(buf[:4])), rec_ranges(_rec(buf[4:])))


def test_adjacent_arena_allocations_are_not_reported():
    from edtr_amd.engine import Arena
    arena = Arena(torch.device("cpu"), 1 << 16)
    a, b = arena.alloc((64,), torch.float32), arena.alloc((3, 5), torch.bfloat16)
    c = arena.alloc((16, 16), torch.float32)
    assert tensor_range(a)[1] == tensor_range(b)[0] and b.data_ptr() + Arena.ALIGN == c.data_ptr()
    A, B, C = (rec_ranges(_rec(t)) for t in (a, b, c))
    assert not ranges_overlap(A, B) and not ranges_overlap(B, A) and not ranges_overlap(A | C, B) and not ranges_overlap(B, A | C)
    arena.free(b)                                                   # the hole goes to the next tensor that fits: now they do meet
    d = arena.alloc((100,), torch.uint8)
    assert ranges_overlap(rec_ranges(_rec(d)), B) == rec_ranges(_rec(d))


def test_nested_keep_and_empty_tensors():
    x, y, z = torch.zeros(4), torch.zeros(6), torch.zeros(5)
    empty = torch.zeros(0)
    r = _rec(object(), ((object(), x), (None, [y, 3, (z,)])), empty, 2.5, "s")
    assert rec_ranges(r) == {tensor_range(x), tensor_range(y), tensor_range(z)}
    assert rec_ranges(_rec()) == set() and rec_ranges(_rec(empty, None)) == set()
    from edtr_amd import ops
    attn, mlp = _rec(object(), x), _rec(object(), y, z)
    fused = ops.Rec(None, (), (attn.keep, mlp.keep), "swin.layer")      # the shape of ops.make_swin_layer's keep
    assert rec_ranges(fused) == rec_ranges(attn) | rec_ranges(mlp)


def test_ranges_overlap_sweep():
    assert ranges_overlap({(0, 10)}, {(10, 20)}) == set() and ranges_overlap({(10, 20)}, {(0, 10)}) == set()      # half-open
    assert ranges_overlap({(0, 11)}, {(10, 20)}) == {(0, 11)}
    assert ranges_overlap({(50, 60)}, {(0, 100), (10, 20), (30, 40)}) == {(50, 60)}       # a long range behind shorter, later ones
    assert ranges_overlap({(5, 6), (25, 26), (40, 41)}, {(0, 10), (20, 30)}) == {(5, 6), (25, 26)}
    assert ranges_overlap({(0, 5)}, {(0, 5)}) == {(0, 5)}
    assert ranges_overlap({(0, 5)}, set()) == set() and ranges_overlap(set(), {(0, 5)}) == set()
    # against the quadratic definition on a pseudo-random set
    g = torch.Generator().manual_seed(11)
    s = torch.randint(0, 4000, (300,), generator=g).tolist()
    n = torch.randint(1, 40, (300,), generator=g).tolist()
    R = [(a, a + b) for a, b in zip(s, n)]
    A, B = set(R[:150]), set(R[150:])
    assert ranges_overlap(A, B) == {a for a in A if any(a[0] < b[1] and b[0] < a[1] for b in B)}


# ---------------------------------------------------------------------------------------------------------------------
# the two lanes of the denoise step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ENGINES, ids=lambda c: "-".join(str(v) for v in c))
def test_fork_and_join_bracket_the_controlnet(engines, case):
    eng, _ = engines(case)
    prog = eng.step_prog
    f, j = _span(prog)                                               # exactly one fork, one join, in that order
    assert len(prog.lanes) == len(prog.recs)
    # the mark still points at the first ControlNet launch although sums_slot() put gn.zero_pool at index 0 and moved the marks
    assert prog.lanes[f] == 1 and prog.lanes[f - 1] == 0
    assert prog.recs[0].name == "gn.zero_pool" and prog.lanes[0] == 0
    assert sum(r.name == "gn.zero_pool" for r in prog.recs) == 1
    assert [i for i, ln in enumerate(prog.lanes) if ln == 1 and not f <= i < j] == []
    assert set(prog.lanes) == {0, 1}
    assert _lane_recs(prog, 1) and _lane_recs(prog, 0)               # two branches: both lanes have work inside the span
    assert set(eng.ctx_prog.lanes) <= {0} and not eng.ctx_prog.marks


@pytest.mark.parametrize("case", ENGINES, ids=lambda c: "-".join(str(v) for v in c))
def test_lanes_touch_no_common_memory_between_fork_and_join(engines, case):
    """Weights included: the two networks have their own.  An arena hole that lane 0 reuses while lane 1 still reads it, or a
    buffer both lanes write, shows here as an overlap."""
    eng, _ = engines(case)
    shared = {rg: names for rg, names in _lane_overlap(eng).items() if not set(names) <= set(LANES_MAY_SHARE)}
    assert shared == {}, f"{len(shared)} lane-1 ranges are touched by lane 0 between fork and join: {sorted(shared.items())[:8]}"


@pytest.mark.parametrize("case", ENGINES, ids=lambda c: "-".join(str(v) for v in c))
def test_lane0_stays_out_of_the_controlnet_arena(engines, case):
    eng, _ = engines(case)
    assert eng.arena_cn is not eng.arena and eng.arena_cn.chunks and eng.arena.chunks
    assert not ranges_overlap(_chunks(eng.arena), _chunks(eng.arena_cn))
    hit = ranges_overlap(_union(_lane_recs(eng.step_prog, 0)), _chunks(eng.arena_cn))
    assert hit == set()
    # and the ControlNet does work there (the rule above is not vacuous)
    assert ranges_overlap(_union(_lane_recs(eng.step_prog, 1)), _chunks(eng.arena_cn))


@pytest.mark.parametrize("case", ENGINES, ids=lambda c: "-".join(str(v) for v in c))
def test_lane1_reads_of_lane0s_arena_what_was_written_before_the_fork(engines, case):
    """What a ControlNet launch uses inside lane 0's arena lies inside a tensor that a launch before the fork, or the context
    program, uses: the NHWC input of conv_in, the time rows res.conv1 reads, the cross-attention K / V^T of flash_attn64 (views of
    the context program's outputs, hence "inside") and, on the fp32 stream, the operand of split_operand.  With the lane rule above
    (lane 0 touches none of them inside the span) they are read-only while the branches run."""
    eng, _ = engines(case)
    prog = eng.step_prog
    f, _j = _span(prog)
    before = _union(prog.recs[:f]) | _union(eng.ctx_prog.recs)
    one = _lane_recs(prog, 1)
    borrowed = ranges_overlap(_union(one), _chunks(eng.arena))
    stray = {rg: sorted({r.name for r in one if rg in rec_ranges(r)}) for rg in borrowed if not _inside(rg, before)}
    assert stray == {}
    readers = {r.name for r in one if rec_ranges(r) & borrowed}
    assert borrowed and readers <= {"conv_in", "res.conv1", "flash_attn64", "split_operand"}, readers


@pytest.mark.parametrize("case", ENGINES, ids=lambda c: "-".join(str(v) for v in c))
def test_groupnorm_accumulator_slots_are_disjoint_and_pooled(engines, case):
    eng, handed = engines(case)
    prog = eng.step_prog
    pool = tensor_range(prog.sums_pool)
    slots = sorted(tensor_range(t) for t in handed)
    assert len(slots) == prog.sums_used > 0
    assert all(pool[0] <= s and e <= pool[1] for s, e in slots)
    assert all(slots[k][1] <= slots[k + 1][0] for k in range(len(slots) - 1)), "two sums_slot() results overlap"
    assert all(e - s == eng.B * 32 * 2 * 8 for s, e in slots)
    # the launches use the pool through these slots only (the zeroing launch aside), and every slot handed out is used
    used = ranges_overlap(_union(prog.recs[1:]), {pool})
    assert used == set(slots)
    assert rec_ranges(prog.recs[0]) == {pool}
    # the pool is no arena memory (it is live from the first launch: see Program.sums_slot)
    assert not ranges_overlap({pool}, _chunks(eng.arena) | _chunks(eng.arena_cn))


def test_one_arena_for_both_lanes_fails_the_lane_rule(models, monkeypatch):
    """The rule has teeth: hand both emitters the SAME arena (as the step program was built before the ControlNet got its own) and
    lane 0 reuses holes the ControlNet's launches still use."""
    import edtr_amd.model.cldm as cldm_mod
    from edtr_amd.engine import Arena
    one = Arena(torch.device("cpu"))
    monkeypatch.setattr(cldm_mod, "Arena", lambda dev: one)
    eng, _ = _build_engine(models("fast"), 2, 16, 16)
    assert eng.arena is eng.arena_cn
    assert len(_lane_overlap(eng)) > 0
    monkeypatch.undo()
    eng, _ = _build_engine(models("fast"), 2, 16, 16)
    assert eng.arena is not eng.arena_cn and _lane_overlap(eng) == {}


# ---------------------------------------------------------------------------------------------------------------------
# the two engine slots
# ---------------------------------------------------------------------------------------------------------------------
def _slot_engines(cldm, slot):
    cldm.engine_slot = slot
    try:
        return (cldm.cldm_engine(2, 16, 16, 77), cldm.vae_engine("encode", 2, 128, 128), cldm.vae_engine("decode", 2, 16, 16),
                cldm.vae_engine("decode", 1, 40, 40, 16))
    finally:
        cldm.engine_slot = 0


def _programs(eng):
    return [eng.step_prog, eng.ctx_prog] if hasattr(eng, "step_prog") else [eng.prog]


def _io(eng):
    names = ("x_in", "hint_in", "t_in", "ctx_in", "eps_out") if hasattr(eng, "step_prog") else ("inp", "out")
    return {tensor_range(getattr(eng, n)) for n in names}


@pytest.mark.parametrize("precision", ["fast", "hybrid"])
def test_two_slots_share_only_the_weight_store(models, precision):
    """bench.py --inflight 2 replays slot 0 and slot 1 on two streams at once: whatever both reach must be read-only, i.e. a
    tensor of the packed weight store (the hybrid mode: of the root store or its sibling format)."""
    cldm = models(precision)
    s0, s1 = _slot_engines(cldm, 0), _slot_engines(cldm, 1)
    assert _slot_engines(cldm, 0)[0] is s0[0] and _slot_engines(cldm, 1)[3] is s1[3]           # cached per slot
    assert s0[3].nan_probe is not None and s0[2].nan_probe is None                              # the last one is the tiled form
    weights = {tensor_range(t) for t in cldm._weights.tensors()}
    for a, b in zip(s0, s1):
        assert a is not b and type(a) is type(b)
        ra, rb = (_union(r for p in _programs(e) for r in p.recs) for e in (a, b))
        both = ranges_overlap(ra, rb) | ranges_overlap(rb, ra)
        assert both, "the slots share their weights"
        outside = sorted(rg for rg in both if not _inside(rg, weights))
        assert outside == [], f"{len(outside)} of {len(both)} ranges that both slots use are no weights"
        mem = [_chunks(e.arena) | (_chunks(e.arena_cn) if hasattr(e, "arena_cn") else set()) |
               {tensor_range(p.sums_pool) for p in _programs(e) if p.sums_pool is not None} | _io(e) for e in (a, b)]
        assert not ranges_overlap(mem[0], mem[1]) and not ranges_overlap(mem[0] | mem[1], weights)
        assert len(_io(a)) == len(_io(b)) == (5 if hasattr(a, "step_prog") else 2)
        assert not ranges_overlap(_io(a), _io(b))
