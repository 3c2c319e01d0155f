#!/usr/bin/env python
"""Drop-in for the reference's train.py (``python scripts/train.py CONFIG.json``); see zett_amd/train_cli.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zett_amd.train_cli import main  # noqa: E402

if __name__ == "__main__":
    main()
