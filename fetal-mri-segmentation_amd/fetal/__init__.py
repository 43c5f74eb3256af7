"""CLI package name of the reference (`python -m fetal.train_fetal`, `python -m fetal.predict`).  Here: `fetal.utils` (scans folder ->
data file, reference fetal/utils.py) and `fetal.experiments` (the adversarial / semi-supervised entry points).  The reference's other
CLI modules and `fetal/config_utils.py` are used unchanged from the reference checkout; see INTEGRATION.md for the overlay recipe."""
