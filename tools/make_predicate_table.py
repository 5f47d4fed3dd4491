"""Records tests/golden/launch_predicates.json: what ops.gn_in_conv_ok and ops.subpixel_ok answer over the grid of
tests/test_host_logic.py (predicate_cases), one bit per case and per switch setting, as answered by a checkout of the commit BEFORE a
change to the predicates — never by the code under test.

    git worktree add /tmp/parent <commit>
    python tools/make_predicate_table.py <commit> /tmp/parent

The checkout goes first on sys.path, so `edtr_amd` is the old commit's; only the grid, the settings and the bit order (the test
module) come from this tree.  A commit whose predicates ask the library needs EDTR_AMD_LIB = a built library of its ABI."""
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main() -> None:
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    commit, tree = sys.argv[1], os.path.abspath(sys.argv[2])
    head = subprocess.check_output(["git", "-C", tree, "rev-parse", "HEAD"], text=True).strip()
    if head != subprocess.check_output(["git", "-C", ROOT, "rev-parse", commit], text=True).strip():
        sys.exit(f"{tree} is at {head}, not at {commit}")
    sys.path[:] = [tree] + [p for p in sys.path if os.path.abspath(p or ".") != ROOT]
    import edtr_amd.ops as old_ops
    assert os.path.abspath(old_ops.__file__).startswith(tree + os.sep), "edtr_amd must come from the checkout, not from this tree"
    spec = importlib.util.spec_from_file_location("predicate_cases", os.path.join(ROOT, "tests", "test_host_logic.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    cases = T.predicate_cases()
    settings = {}
    for name, env in T.PREDICATE_SETTINGS.items():
        for k in T.PREDICATE_SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        settings[name] = {k: {"accepted": sum(v), "bits": T.bits_hex(v)} for k, v in T.predicate_answers(old_ops, cases).items()}
        print(name, {k: v["accepted"] for k, v in settings[name].items()}, file=sys.stderr)
    with open(T.PREDICATE_TABLE, "w") as fh:
        json.dump({"recorded_from": head, "cases": {k: len(v) for k, v in cases.items()}, "settings": settings}, fh, sort_keys=True,
                  separators=(",", ":"))
        fh.write("\n")
    print(f"{os.path.getsize(T.PREDICATE_TABLE)} bytes", file=sys.stderr)


if __name__ == "__main__":
    main()
