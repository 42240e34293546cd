"""The reference's `env/` package on the device: the lidar navigation task without ROS and Gazebo."""
from .navsim import (DEFAULTS, STATUS_NAMES, LidarNavSim, NavStep, NavWorld, beam_table, collect, nav_scan,  # noqa: F401
                     random_command)
