"""Tube learning: train a tube MLP on the ROM tracking data that scripts/collect_trajectory_data.py records:
trainer.HipTubeTrainer for one model, sweep.HipTubeSweep for K models of one shape in the same two launches per step -- one
training path (trainer.TubeTraining, one C trainer) with one member or K;
device_data builds the datasets on the device, from records or straight from the ROM simulator."""
from .device_data import SimTubeDataset, build_rows, from_records  # noqa: F401
