"""The reference's `env/` package on the device: the lidar navigation task without ROS and Gazebo, with
the continuous command of env/gazebo.py (navsim.py) and as the discrete task of env/env.py (env.py), and an A* expert that
drives either (expert.py)."""
from .env import DiscreteLidarNavSim, Env  # noqa: F401
from .expert import AStarExpert, PlanGrid  # noqa: F401
from .navsim import (DEFAULTS, STATUS_NAMES, LidarNavSim, NavStep, NavWorld, beam_table, collect, nav_scan,  # noqa: F401
                     random_command)
