"""Writes tests/golden/pack_hashes.json: per case of tests/pack_golden_cases.py the checksums of the packed problem, its sizes and the
first LM trials, as the library built in this tree produces them.  Run it at the commit whose behaviour is to be kept; afterwards
tests/test_gpu_pack_golden.py holds every later commit to the file, word for word.
  python tools/pack_hash_golden.py [output.json [case ...]]     (cases given: only those are recorded, into the file as it is)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("nr-slam_amd/py", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import pack_golden_cases as G
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "pack_hashes.json")
res = {}
if sys.argv[2:]:
    with open(out) as fh:
        res = json.load(fh)
for name in sys.argv[2:] or G.CASES:
    res[name] = G.record(name)
    print(name, "ok", flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as fh:
    json.dump(res, fh, indent=1, sort_keys=True)
    fh.write("\n")
print("wrote", out)
