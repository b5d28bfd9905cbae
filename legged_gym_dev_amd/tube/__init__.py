"""Tube learning: train a tube MLP on the ROM tracking data that scripts/collect_trajectory_data.py records."""
