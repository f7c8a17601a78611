"""`bench.py --mode train` with the deterministic training mode (train.set_deterministic) switched on or off - bench.py has no switch for
it.  Same workload, same JSON result line, preceded by one line that names the mode.

    python tools/train_det_bench.py [--deterministic 0|1] [bench.py arguments, e.g. --steps 20 --warmup 5 --img-tune]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    argv, det = sys.argv[1:], True
    if "--deterministic" in argv:
        i = argv.index("--deterministic")
        det = bool(int(argv[i + 1]))
        del argv[i:i + 2]
    from candidate_reranking_cir_amd import train
    train.set_deterministic(det)
    import bench
    print(json.dumps({"deterministic": train.deterministic()}), flush=True)
    sys.argv = ["bench.py", "--mode", "train", "--gpus", "1", "--no-cpu-baseline"] + argv
    bench.main()


if __name__ == "__main__":
    main()
