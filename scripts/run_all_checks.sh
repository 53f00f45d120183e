#!/bin/bash
# Everything a reviewer would run on a GPU box, in order: build, CPU suite, GPU parity suite, smoke, the bench with every side measurement.
set -e
cd "$(dirname "$0")/.."
python __graft_entry__.py smoke                # build() then smoke() on cuda:0
python -m pytest tests -q -m "not gpu"
python -m pytest tests -q -m gpu
python bench.py --full
