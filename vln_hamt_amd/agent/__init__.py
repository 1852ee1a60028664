"""The part of a finetune rollout every agent of the reference shares (R2R, R2R-back, CVDN, REVERIE's action side): the per-step action
choice and losses on the device, and (nav_graph) what they read from the navigation graph: teacher lookup, back-track mask, reward
shaping, metrics; REVERIE's own step (the object STOP column, `ref_loss`, the predicted object) is `ReverieRolloutRecorder`.  The agents
themselves and the simulator are out of scope; their optimiser pair (optim) is here.  (obs) gathers the observations a step feeds the
model -- candidates, STOP, the remaining views, the history views -- from a viewpoint store on the device; (obj_obs) REVERIE's candidate objects
of the viewpoint stood on, from an object store over the same rows."""
from .nav_graph import GoalSetEpisodes, NavEpisodes, NavGraphs, ReturnEpisodes
from .obj_obs import ObjEpisodes, ObjObservation, ObjStore, build_obj_tables, goal_objects
from .obs import ObsEpisodes, ObsStore, Observation
from .optim import AgentOptimizers, build_agent_optimizers
from .recorder import RolloutRecorder
from .recorder_reverie import ReverieRolloutRecorder

__all__ = ["AgentOptimizers", "GoalSetEpisodes", "NavEpisodes", "NavGraphs", "ObjEpisodes", "ObjObservation", "ObjStore", "ObsEpisodes", "ObsStore",
           "Observation", "ReturnEpisodes", "ReverieRolloutRecorder", "RolloutRecorder", "build_agent_optimizers", "build_obj_tables",
           "goal_objects"]
