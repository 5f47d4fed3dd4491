"""The launch programs are built entirely on the host, so "this change moves no launch" is checked exactly and without a GPU: every
program below is rebuilt on the CPU, written out record by record (edtr_amd.testing.program_signature: names, shapes, every struct
field and scalar, pointers as arena offsets or first-appearance numbers) and compared with tests/golden/program_signatures.json,
which tools/make_program_signatures.py recorded from the commit BEFORE the change under test (the emitter's plan).

A change that moves emission on purpose re-records the table from its own parent and says so.  A mismatch names the first record
that differs and leaves the rebuilt listing in the test's temporary directory; the recorder's `--dump DIR` writes the recorded
listings, so the two can be diffed line by line.

Every group of programs is built in a fresh child process with a clean EDTR_* environment plus the group's own switches (some
switches are read once at import or on the first plan); the children of all groups run side by side.  The same children ask the
library's planners about every record that has one: what Python promised at emission, the library must take at launch."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TABLE = os.path.join(HERE, "golden", "program_signatures.json")

CLDM_TINY = [(2, 16, 16), (1, 24, 16), (2, 32, 32), (16, 64, 64)]
VAE_TINY = [("encode", 2, 64, 64), ("decode", 2, 8, 8), ("encode", 1, 128, 128, 32), ("decode", 1, 48, 48, 16)]
CLDM_FULL = [(1, 64, 64), (2, 64, 64), (4, 64, 64), (8, 64, 64), (16, 64, 64), (1, 128, 128), (8, 32, 32)]
VAE_FULL = [("encode", 8, 512, 512), ("encode", 1, 1024, 1024, 256), ("decode", 8, 64, 64), ("decode", 1, 128, 128), ("decode", 1, 128, 128, 64)]
MODES = ("fast", "mixed", "high", "hybrid")
SWITCHES = {"ktail0": {"EDTR_KTAIL": "0"}, "invariant": {"EDTR_AMD_BATCH_INVARIANT": "1"}, "gn_in_conv0": {"EDTR_GN_IN_CONV": "0"},
            "subpixel0": {"EDTR_SUBPIXEL": "0"}, "lin320_ffn0": {"EDTR_LIN320": "0", "EDTR_FFN": "0"},
            "gn_concat_stats0": {"EDTR_GN_CONCAT_STATS": "0"}, "gn_splitk_stats0": {"EDTR_GN_SPLITK_STATS": "0"}}

# group -> (environment switches, configuration, precision modes, CldmEngine shapes, VaeEngine arguments, with _small_engines()?)
GROUPS = {"tiny": ({}, "tiny", MODES, CLDM_TINY, VAE_TINY, True),
          "full.fast": ({}, "sd21", ("fast",), CLDM_FULL, VAE_FULL, False)}
GROUPS.update({f"full.{m}": ({}, "sd21", (m,), [(8, 64, 64)], [("encode", 8, 512, 512), ("decode", 8, 64, 64)], False) for m in MODES[1:]})
GROUPS.update({f"switch.{k}": (env, "sd21", ("fast",), [(8, 64, 64)], [("decode", 8, 64, 64)], False) for k, env in SWITCHES.items()})
ORDER = sorted(GROUPS, key=lambda g: (not g.startswith("full"), g))      # the long ones first


def _small_engines():
    """{name: (launch records, arenas)} of the SwinIR and CLIP text engines and of the three hand-built programs of
    tests/test_gpu_e2e.py::test_deferred_groupnorm_falls_back_to_its_apply_launch (emission only)."""
    import torch
    import edtr_amd.ops as ops_mod
    from edtr_amd import synth
    from edtr_amd.engine import Act, Arena, Emitter, Program, WeightStore
    from edtr_amd.model.clip import FrozenOpenCLIPEmbedder, _TextEngine
    from edtr_amd.model.params import skip_init
    from edtr_amd.model.swinir import SwinIR, _SwinEngine
    out = {}
    for name, cfg in (("swinir.small", synth.swinir_small_config()), ("swinir.full", synth.swinir_config())):
        with skip_init():
            sw = SwinIR(**cfg)
        sw.compute_dtype = torch.bfloat16
        eng = _SwinEngine(sw, 1, 64, 64, graph=False)
        out[name] = (eng.prog.recs, [eng.arena])
    with skip_init():
        clip = FrozenOpenCLIPEmbedder(**synth.clip_small_config())
    clip.compute_dtype = torch.bfloat16
    eng = _TextEngine(clip, 4)
    out["clip.small"] = (eng.prog.recs, [eng.arena])
    dev = torch.device("cpu")
    B, H, C, N = 2, 80, 128, 128
    params = {"n.weight": torch.ones(C), "n.bias": torch.zeros(C), "c.weight": torch.zeros(N, C, 3, 3), "c.bias": torch.zeros(N)}
    for case in ("stride2", "splitk", "fusable"):
        for defer in (False, True):
            prog, arena = Program("t"), Arena(dev, 1 << 26)
            em = Emitter(prog, arena, WeightStore(params, torch.bfloat16, dev), torch.bfloat16)
            xa = Act(arena.alloc((B * H * H, C), torch.bfloat16), B, H, H, C)
            h = em.group_norm(xa, "n.", 1e-6, True, conv_n=N if defer else 0)
            real = ops_mod.gn_in_conv_ok
            if defer and case == "splitk":
                ops_mod.gn_in_conv_ok = lambda *a, **k: False
            try:
                em.conv(h, "c.", name="res.conv1", **(dict(stride=2, pad_tl=0) if case == "stride2" else {}))
            finally:
                ops_mod.gn_in_conv_ok = real
            out[f"deferred_gn.{case}.{'deferred' if defer else 'plain'}"] = (prog.recs, [arena])
    return out


PLANNERS = ("edtr_igemm", "edtr_ffn", "edtr_lin320", "edtr_flash_attn64")     # launches with an edtr_*_plan that answers without a device
PLANNED = {}            # group -> {"asked": {launch: records}, "refused": [descriptions]}, filled by finish_child


def ask_planners(recs, planned: dict) -> None:
    """The library's own answer for every record of PLANNERS' launches: counted in planned["asked"], a refusal described in
    planned["refused"]."""
    from edtr_amd import lib
    for r in recs:
        fn = getattr(r.fn, "__name__", "")
        if fn in PLANNERS:
            answer = getattr(lib.load(), fn + "_plan")(r.args[0], *((None,) if fn == "edtr_flash_attn64" else ()))
            planned["asked"][fn] = planned["asked"].get(fn, 0) + 1
            if answer < 0:
                planned["refused"].append(f"{fn} {answer}: {r.name} {r.tag}")


def build_group(group: str):
    """Yields (program name, launch records, arenas) for every program of ``group``, built on the CPU in this process."""
    import torch
    from edtr_amd import synth
    from edtr_amd.model import ControlLDM
    from edtr_amd.model.cldm import CldmEngine, VaeEngine
    from edtr_amd.model.params import skip_init
    _, config, modes, cldm_shapes, vae_args, small = GROUPS[group]
    cfg = synth.tiny_config() if config == "tiny" else synth.sd21_config()
    with skip_init():                  # emission reads shapes only: no state dict is loaded
        model = ControlLDM(**cfg).eval()
    model.compute_dtype = torch.bfloat16
    for mode in modes:
        model.precision = model.controlnet.precision = model.unet.precision = mode
        model.release_engines()
        for shape in cldm_shapes:
            eng = CldmEngine(model, *shape, 77)
            key = f"{config}.{mode}.cldm." + "x".join(map(str, shape))
            yield key + ".context", eng.ctx_prog.recs, [eng.arena, eng.arena_cn]
            yield key + ".step", eng.step_prog.recs, [eng.arena, eng.arena_cn]
        for args in vae_args:
            eng = VaeEngine(model, *args)
            yield f"{config}.{mode}.vae." + ".".join(map(str, args)), eng.prog.recs, [eng.arena]
    if small:
        for name, (recs, arenas) in _small_engines().items():
            yield name, recs, arenas


def child_main(group: str, dump: str = "") -> None:
    import torch
    from edtr_amd.testing import program_signature, signature_summary
    torch.set_num_threads(2)
    out, planned = {}, {"asked": {}, "refused": []}
    for name, recs, arenas in build_group(group):
        lines = program_signature(recs, arenas)
        ask_planners(recs, planned)
        out[name] = signature_summary(lines)
        if dump:
            os.makedirs(dump, exist_ok=True)
            with open(os.path.join(dump, f"{group}--{name}.txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")
    print("PLANNED " + json.dumps(planned, sort_keys=True))
    print("SIGNATURES " + json.dumps(out, sort_keys=True))


def start_child(group: str, argv, pythonpath=None, dump: str = "") -> subprocess.Popen:
    """A fresh interpreter that runs ``argv + [group, dump]`` with the EDTR_* variables cleared, then the group's switches set."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("EDTR_")}
    env.update(GROUPS[group][0])
    if os.environ.get("EDTR_AMD_LIB"):         # (the recorder points an old commit's Python at a built library)
        env["EDTR_AMD_LIB"] = os.environ["EDTR_AMD_LIB"]
    env["PYTHONPATH"] = os.pathsep.join([pythonpath or ROOT] + [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    return subprocess.Popen([sys.executable] + list(argv) + [group, dump], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def finish_child(group: str, proc: subprocess.Popen) -> dict:
    out, err = proc.communicate()
    lines = [ln for ln in out.splitlines() if ln.startswith("SIGNATURES ")]
    if proc.returncode != 0 or len(lines) != 1:
        raise RuntimeError(f"{group}: the child process failed ({proc.returncode})\n{err[-4000:]}")
    PLANNED[group] = json.loads(next(ln for ln in out.splitlines() if ln.startswith("PLANNED "))[len("PLANNED "):])
    return json.loads(lines[0][len("SIGNATURES "):])


def run_groups(argv, pythonpath=None, dump: str = "", parallel: int = 4):
    """Yields (group, {program: summary}) for every group, at most ``parallel`` children at a time (a full-width model is 5 GB)."""
    waiting, running = list(ORDER), []
    while waiting or running:
        while waiting and len(running) < parallel:
            g = waiting.pop(0)
            running.append((g, start_child(g, argv, pythonpath, dump)))
        g, proc = running.pop(0)
        yield g, finish_child(g, proc)


@pytest.fixture(scope="module")
def rebuilt(tmp_path_factory):
    dump = str(tmp_path_factory.mktemp("listings"))
    return dict(run_groups([os.path.abspath(__file__)], dump=dump)), dump


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as fh:
        return json.load(fh)


def _first_difference(new_file: str, group: str, name: str, want: dict, got: dict) -> str:
    """Names the first record whose hash differs from the recorded one and quotes it from the new listing — and from the recorded
    listing too where that is at hand (EDTR_SIGNATURE_LISTINGS=DIR, written by the recorder's --dump)."""
    old_h, new_h = want["record_hashes"], got["record_hashes"]
    i = next((k for k in range(min(len(old_h), len(new_h)) // 6) if old_h[6 * k:6 * k + 6] != new_h[6 * k:6 * k + 6]), None)
    where = f"(new listing: {new_file})"
    if i is None:
        return f"the first {min(want['records'], got['records'])} records agree; recorded {want['records']}, rebuilt {got['records']} {where}"
    with open(new_file) as fh:
        text = f"first differing record {i}:\n  rebuilt:  {fh.read().splitlines()[i]}"
    old_file = os.path.join(os.environ.get("EDTR_SIGNATURE_LISTINGS", ""), f"{group}--{name}.txt")
    if os.path.exists(old_file):
        with open(old_file) as fh:
            text += f"\n  recorded: {fh.read().splitlines()[i]}"
    return f"{text}\n{where}"


@pytest.mark.parametrize("group", ORDER)
def test_programs_match_the_recorded_signatures(group, rebuilt, table):
    got, dump = rebuilt
    want = table["groups"][group]
    assert sorted(got[group]) == sorted(want), "the set of programs changed"
    for name in sorted(want):
        if got[group][name] != want[name]:
            counts = {k: (want[name]["launches"].get(k, 0), got[group][name]["launches"].get(k, 0))
                      for k in set(want[name]["launches"]) | set(got[group][name]["launches"])}
            moved = {k: v for k, v in sorted(counts.items()) if v[0] != v[1]}
            pytest.fail(f"{group} / {name}: records {want[name]['records']} -> {got[group][name]['records']}, launch counts that moved "
                        f"(recorded, rebuilt): {moved or 'none'}\n"
                        + _first_difference(os.path.join(dump, f"{group}--{name}.txt"), group, name, want[name], got[group][name]))


def test_the_library_admits_every_launch_the_emitters_promise(rebuilt):
    """Every edtr_igemm, edtr_ffn, edtr_lin320 and edtr_flash_attn64 record of every rebuilt program, asked of the library's own planner
    (no device): nothing is refused.  This is what holds the Python-side promises (ops.gn_in_conv_ok, subpixel_ok, gn_fusable,
    choose_splitk, ffn_ok, lin320_ok, the K tails) inside the library's rules."""
    assert sorted(PLANNED) == sorted(GROUPS)
    asked = {fn: sum(p["asked"].get(fn, 0) for p in PLANNED.values()) for fn in PLANNERS}
    print("records asked of the planners:", asked)
    assert all(asked.values()), asked
    refused = [f"{g}: {what}" for g in ORDER for what in PLANNED[g]["refused"]]
    assert not refused, "%d records refused, the first: %r" % (len(refused), refused[:5])


def test_the_table_covers_every_switch_and_mode(table):
    assert sorted(table["groups"]) == sorted(GROUPS)
    assert len(table["recorded_from"]) >= 7
    base = table["groups"]["full.fast"]["sd21.fast.cldm.8x64x64.step"]["sha256"]
    for k in SWITCHES:          # a switch that moved nothing would pin nothing
        sw = table["groups"][f"switch.{k}"]
        assert any(v["sha256"] != table["groups"]["full.fast"].get(n, {}).get("sha256") for n, v in sw.items()), k
    assert len({table["groups"][f"full.{m}"][f"sd21.{m}.cldm.8x64x64.step"]["sha256"] for m in MODES}) == len(MODES) and base


def test_the_emitter_keeps_no_state_about_its_last_launch():
    """By-products of a launch are returned (engine.Out, the Act of conv), and the measured policy is asked in one place."""
    import glob
    import re
    src = {p: open(p).read() for p in glob.glob(os.path.join(ROOT, "edtr_amd", "**", "*.py"), recursive=True)}
    for gone in ("last_gnp", "last_gn_slot", "last_row_stats", "gnp_into_done", "add_stats_done"):
        assert not [p for p, s in src.items() if gone in s], gone
    engine = src[os.path.join(ROOT, "edtr_amd", "engine.py")]
    init = engine.split("class Emitter:")[1].split("    def parts_for")[0]
    assert not re.search(r"self\.(last_|\w+_done\b)", init)
    assert len(re.findall(r"ops\.choose_splitk\(", engine)) == 1 and len(re.findall(r"ops\.gn_in_conv_ok\(", engine)) == 1


if __name__ == "__main__":
    child_main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "")
