"""`from iwls import iwls` for the reference's unchanged code/main.py (main.py:15): see INTEGRATION.md."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from riemannhamiltonianmontecarlo_amd.iwls import iwls  # noqa: E402,F401
