"""Write tests/golden/transformer_cache_small.npz: the outputs of the reference's OWN codec Transformer (encoder_modules/transformer.py) on
seeded weights and inputs - offline non-causal, offline causal, and the cache mode (DynamicCache) over the chunks (5, 7, 1, 11).  Data
only: the weights are regenerated from the stored seed (tests/transformer_stream_ref.golden_inputs).  Needs the reference tree.

    python tools/gen_golden_transformer_cache.py [--seed 4201]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import transformer_stream_ref as TR  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=4201)
    args = ap.parse_args()
    arrays = TR.reference_golden(args.seed)
    os.makedirs(os.path.dirname(TR.GOLDEN), exist_ok=True)
    np.savez_compressed(TR.GOLDEN, **arrays)
    print(f"wrote {TR.GOLDEN}: " + ", ".join(f"{k} {v.shape}" for k, v in arrays.items()))
