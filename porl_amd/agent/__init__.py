"""Agents.  `GoalConditionedBC` is exported here; the other agents are imported from their modules (agent.por, agent.sorl)."""


def __getattr__(name):
    if name == "GoalConditionedBC":            # resolved on first use: importing the package stays free of torch
        from .goal_bc import GoalConditionedBC
        return GoalConditionedBC
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["GoalConditionedBC"]
