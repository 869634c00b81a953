"""A fresh process for tests/test_gpu_round_cases.py: the whole round catalogue (oracle/roundcases.py) through the engine's one continuous stream under
whatever ZGPU_FW_RING / ZGPU_FAST_KEEP / ZGPU_FAST_FORCE_ROUNDS the parent put into the environment -- knobs the library reads once per process.
Prints one line per case and level whose bytes are not the golden file's ("DIFFERS name cfg"), then "DONE <runs>".  python -m round_cases_child"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    import zlib_amd
    from zlib_amd import gpu
    from oracle import roundcases as RC
    with open(os.path.join(ROOT, "tests", "golden", "round_kat.json")) as f:
        gold = json.load(f)["cases"]
    eng = zlib_amd.Engine(0)
    runs = 0
    for c in RC.catalogue():
        for cfg in c.cfgs:
            z = eng.deflate_host(c.data, RC.level_of(cfg), flags=gpu.F_FINAL | gpu.F_CONTINUOUS)
            runs += 1
            if [len(z), hashlib.sha256(z).hexdigest()[:16]] != gold[c.name]["out"][cfg]:
                print("DIFFERS", c.name, cfg, flush=True)
    eng.close()
    print("DONE", runs, flush=True)


if __name__ == "__main__":
    main()
