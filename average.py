#!/usr/bin/env python
"""`python average.py --inputs PREFIX ... --output PREFIX` (from the repository root): mtn_amd.average with the same flags."""
from mtn_amd.average import main

if __name__ == "__main__":
    main()
