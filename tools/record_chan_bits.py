"""tools/record_bits.py chan [--check] [--out FILE]."""
import sys

from record_bits import main

if __name__ == "__main__":
    sys.exit(main("chan"))
