"""Writes tests/golden/features_structure.npz (data only): the reference's own create_subgraphs on the multi-edge graphs of
tests/feature_cases.py - repeated (s, t) entries, reversed repeats and pre-existing self loops - at the four configurations
of feature_cases.MULTI_EDGE_CONFIGS.  The reference is imported in place by oracle/make_golden.py (under oracle/pyg_shim);
a case on which the oracle (oracle/ref_features.py) disagrees with it is not written.  Same ragged int32 layout as the other
features_*.npz fixtures (conftest.FeatureCases reads it).

    python tools/make_golden_feature_structure.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import make_golden as mg  # noqa: E402      (run_reference, check_oracle, Pack)
import feature_cases as fc  # noqa: E402


def main():
    pack, bad = mg.Pack(), []
    for cfg in fc.MULTI_EDGE_CONFIGS:
        for gi, (n, s, t) in enumerate(fc.MULTI_EDGE_GRAPHS):
            o = mg.run_reference(n, s, t, *cfg)
            if not mg.check_oracle(n, s, t, cfg[0], cfg[1], cfg[2], o):
                bad.append((gi, cfg))
            pack.add(fc.multi_edge_name(gi, cfg), n, s, t, cfg[0], cfg[1], cfg[2], o)
    if bad:
        raise SystemExit("oracle disagrees with the reference on %s" % bad)
    pack.save(os.path.join(mg.OUT, fc.GOLDEN_FILE))


if __name__ == "__main__":
    main()
