#!/usr/bin/env python
"""`python generate.py ...` as run.sh:156-168 calls it (from the repository root): mtn_amd.generate with the same flags."""
from mtn_amd.generate import main

if __name__ == "__main__":
    main()
