"""Regenerate tests/golden/init_demo_seed11.json: the reference model's freshly constructed
state_dict on configs/demo.yaml under torch.manual_seed(11), recorded as one SHA-256 digest per
tensor (the 886,540 parameters themselves would be 3.5 MB). The reference is imported from the
directory given on the command line, never copied:

    python tests/golden/make_init_golden.py --reference <path to the reference checkout>

tests/test_cpu_host.py::test_initial_weights_identical_to_reference_under_same_seed compares the
digests of our modules' initial state_dict with these.
"""
import argparse
import hashlib
import json
import os
import sys

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, 'tests', 'golden', 'init_demo_seed11.json')
SEED = 11


def tensor_digests(state_dict):
    """{key: {shape, dtype, sha256 of the contiguous little-endian bytes}} in state_dict order."""
    out = {}
    for k, v in state_dict.items():
        a = v.detach().cpu().contiguous().numpy()
        out[k] = {'shape': list(a.shape), 'dtype': str(a.dtype), 'sha256': hashlib.sha256(a.tobytes()).hexdigest()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='directory of the reference checkout')
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from project.models.TwoTower.GenericTower import GenericTower as RG
    from project.models.TwoTower.TwoTowerModel import TwoTowerModel as RM
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'demo.yaml')))
    torch.manual_seed(SEED)
    ref = RM(RG(cfg, 'user_tower'), RG(cfg, 'item_tower')).state_dict()
    json.dump({'config': 'demo', 'seed': SEED, 'torch': str(torch.__version__),
               'generator': 'tests/golden/make_init_golden.py (reference import)',
               'tensors': tensor_digests(ref)}, open(OUT, 'w'), indent=1)
    print(f'wrote {OUT}: {len(ref)} tensors')


if __name__ == '__main__':
    main()
