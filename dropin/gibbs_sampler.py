"""`from gibbs_sampler import auxiliary_gibbs` for the reference's unchanged code/main.py (main.py:13): see INTEGRATION.md."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from riemannhamiltonianmontecarlo_amd.gibbs_sampler import auxiliary_gibbs  # noqa: E402,F401
