"""Records tests/golden/program_signatures.json: the signature of every launch program that tests/test_program_signatures_cpu.py
rebuilds, as emitted by a checkout of the commit BEFORE a change to the emitters — never by the code under test.

    git worktree add /tmp/parent <commit>
    EDTR_AMD_LIB=/path/to/libedtr_hip.so python tools/make_program_signatures.py <commit> /tmp/parent [--dump DIR]

The checkout goes first on PYTHONPATH of every child process, so `edtr_amd` is the old commit's; only the list of programs (the
test module) and the canonicaliser (edtr_amd/testing.py: program_signature, which reads nothing but launch records and arena
chunks) come from this tree.  EDTR_AMD_LIB names a built library of the same ABI (emission asks it for tile plans).  The file holds,
per program, the record count, the SHA-256 of the listing, the launches per name and six hex digits of every record's own hash (a
failing test names the first differing record from them); --dump DIR also writes the listings themselves
(EDTR_SIGNATURE_LISTINGS=DIR then lets the failing test quote the recorded line beside the rebuilt one)."""
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(name: str, path: str):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def child(group: str, dump: str) -> None:
    import edtr_amd                                                  # the old commit's package (PYTHONPATH)
    assert not os.path.abspath(edtr_amd.__file__).startswith(ROOT + os.sep), "edtr_amd must come from the checkout, not from this tree"
    load("edtr_amd.testing", os.path.join(ROOT, "edtr_amd", "testing.py"))      # this tree's canonicaliser over the old package
    load("program_signature_cases", os.path.join(ROOT, "tests", "test_program_signatures_cpu.py")).child_main(group, dump)


def main() -> None:
    if len(sys.argv) >= 2 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3])
    args = [a for a in sys.argv[1:] if a != "--dump"]
    dump = sys.argv[sys.argv.index("--dump") + 1] if "--dump" in sys.argv else ""
    if dump:
        args.remove(dump)
    if len(args) != 2 or not os.environ.get("EDTR_AMD_LIB"):
        sys.exit(__doc__)
    commit, tree = args[0], os.path.abspath(args[1])
    head = subprocess.check_output(["git", "-C", tree, "rev-parse", "HEAD"], text=True).strip()
    if head != subprocess.check_output(["git", "-C", ROOT, "rev-parse", commit], text=True).strip():
        sys.exit(f"{tree} is at {head}, not at {commit}")
    T = load("program_signature_cases", os.path.join(ROOT, "tests", "test_program_signatures_cpu.py"))
    groups = {}
    for group, sigs in T.run_groups([os.path.abspath(__file__), "--child"], pythonpath=tree, dump=os.path.abspath(dump) if dump else ""):
        groups[group] = sigs
        print(f"{group}: {len(sigs)} programs, {sum(s['records'] for s in sigs.values())} records", file=sys.stderr)
    with open(T.TABLE, "w") as fh:
        json.dump({"recorded_from": head, "groups": groups}, fh, sort_keys=True, separators=(",", ":"))
        fh.write("\n")
    print(f"{os.path.getsize(T.TABLE)} bytes", file=sys.stderr)


if __name__ == "__main__":
    main()
