"""Optimizers of the training step."""
from .adam import Adam
from .clip import GradClipper
from .sgd import SGD
from .solver import LRSchedule, make_optimizer, param_groups

__all__ = ["Adam", "GradClipper", "SGD", "LRSchedule", "make_optimizer", "param_groups"]
