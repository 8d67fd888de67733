"""Makes tests/golden/estimate_oracle.json: for the inputs tests/estimate_ref.py names, the per-plane Q24 code-length sums and
symbol counts of the oracle's own coder operations (oracle.trace_encode_from_bwt), the size the estimate's formula gives for them
and the size of the oracle's archive.  No GPU is involved: the sums use the library's host build of the cost function
(bce_hip_cost_q24).  Prints the error of the method per input; DESIGN.md section 4.7 quotes the worst."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import estimate_ref as ref  # noqa: E402
import oracle  # noqa: E402


def main():
    vectors = []
    custom = ref.custom_config()
    for cfg_name, cfg in (("default", None), ("scanned", custom)):
        for name, data in ref.inputs():
            n, offset, cost, steps = ref.oracle_sums(data, cfg)
            est = ref.archive_bytes(n, offset, cost, cfg)
            real = len(oracle.compress(data, cfg))
            vectors.append({"name": name, "config": cfg_name, "n": n, "offset": offset, "archive_bytes": est, "oracle_archive_bytes": real,
                            "plane_cost_q24": cost, "plane_steps": steps})
            print("%-16s %-8s n=%8d  estimate %9d  oracle %9d  error %+6d B  %+.3e" % (name, cfg_name, n, est, real, est - real, (est - real) / real))
    worst_abs = max(abs(v["archive_bytes"] - v["oracle_archive_bytes"]) for v in vectors)
    worst_rel = max(abs(v["archive_bytes"] - v["oracle_archive_bytes"]) / v["oracle_archive_bytes"] for v in vectors)
    print("worst absolute error %d B, worst relative error %.3e" % (worst_abs, worst_rel))
    out = {"provenance": "tools/make_estimate_golden.py: oracle.trace_encode_from_bwt ops summed with bce_hip_cost_q24; no GPU code involved",
           "worst_abs_error_bytes": worst_abs, "worst_rel_error": worst_rel, "vectors": vectors}
    with open(ref.GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
