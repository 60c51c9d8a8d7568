"""Optimizers of the training step."""
from .adam import Adam
from .sgd import SGD
from .solver import LRSchedule, make_optimizer, param_groups

__all__ = ["Adam", "SGD", "LRSchedule", "make_optimizer", "param_groups"]
