"""`from metropolis import AMH` for the reference's unchanged code/main.py (main.py:11): see INTEGRATION.md."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from riemannhamiltonianmontecarlo_amd.metropolis import AMH  # noqa: E402,F401
