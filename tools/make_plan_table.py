"""Records tests/golden/igemm_plan_table.json: edtr_igemm_plan's answers for the generated cases of tests/test_igemm_plan_cpu.py, from
the library named by EDTR_AMD_LIB — a build of the commit BEFORE a change to the planner, never the code under test.

    EDTR_AMD_LIB=/path/to/old/libedtr_hip.so python tools/make_plan_table.py <commit the library was built from>

The file holds answers only: one int per case (tile number or error code), the case count and a hash of the generated parameter
structs, and per environment switch setting the answers of up to 40 cases from a fresh process with the switch set (the cases whose
answer the switch moves first, then some it leaves alone)."""
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    lib_path = os.environ.get("EDTR_AMD_LIB")
    if not lib_path or len(sys.argv) != 2:
        sys.exit(__doc__)
    spec = importlib.util.spec_from_file_location("igemm_plan_cases", os.path.join(ROOT, "tests", "test_igemm_plan_cpu.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    cases, pairs = T.generate()
    blobs = T.case_bytes(cases)
    answers = T.child_answers({}, blobs, lib_path)
    assert len(answers) == len(cases)
    switches = {}
    for name, env in T.SWITCH_SETTINGS.items():
        got = T.child_answers(env, blobs, lib_path)
        moved = [i for i in range(len(cases)) if got[i] != answers[i]]
        step = max(1, len(moved) // 32)
        pick = moved[::step][:32] + [i for i in range(0, len(cases), max(1, len(cases) // 8)) if got[i] == answers[i]][:8]
        switches[name] = {"cases": pick, "answers": [got[i] for i in pick]}
        print(f"{name}: {len(moved)} cases move", file=sys.stderr)
    table = {"recorded_from": sys.argv[1], "cases": len(cases), "case_hash": T.case_hash(blobs), "answers": answers,
             "switches": switches}
    with open(T.TABLE, "w") as fh:
        json.dump(table, fh, separators=(",", ":"))
        fh.write("\n")
    unpinned = [r for r in T.RULES if not any(answers[a] != answers[b] for a, b in pairs.get(r, []))]
    print(f"{len(cases)} cases, {os.path.getsize(T.TABLE)} bytes; rules without a pair whose answers differ: {unpinned}", file=sys.stderr)


if __name__ == "__main__":
    main()
