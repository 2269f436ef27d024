#!/usr/bin/env python
"""`python evaluate.py RESULT.json REFERENCE.json` (from the repository root): run.sh's stage 4 on the device, mtn_amd.evaluate."""
from mtn_amd.evaluate import main

if __name__ == "__main__":
    main()
