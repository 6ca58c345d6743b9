"""Records what the reference's own `index_generation` returns into tests/golden/index_generation.json.

    python tools/gen_index_generation_golden.py /path/to/reference/codes

The reference checkout is needed only for this one-off recording: tests/test_stream_schedule.py reads the JSON alone.
Cases: N in {3, 5, 7}, max_n in [N, 12], every crt_i, the four padding modes; keyed "N,max_n,crt_i,mode"."""
import importlib.util
import json
import os
import sys

MODES = ('replicate', 'reflection', 'new_info', 'circle')


def main():
    codes = sys.argv[1]
    spec = importlib.util.spec_from_file_location("reference_data_util", os.path.join(codes, "data", "util.py"))
    ref = importlib.util.module_from_spec(spec)
    for dep in ("cv2",):        # imported at the top of that file, not used by index_generation: an empty stand-in will do
        if importlib.util.find_spec(dep) is None:
            sys.modules[dep] = type(sys)(dep)
    spec.loader.exec_module(ref)
    out = {}
    for n in (3, 5, 7):
        for max_n in range(n, 13):
            for crt in range(max_n):
                for mode in MODES:
                    out["%d,%d,%d,%s" % (n, max_n, crt, mode)] = ref.index_generation(crt, max_n, n, padding=mode)
    dst = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "index_generation.json")
    with open(dst, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(dst, len(out))


if __name__ == "__main__":
    main()
