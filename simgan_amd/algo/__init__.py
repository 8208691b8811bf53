from .ppo import PPO  # noqa: F401
from .a2c_acktr import A2C_ACKTR  # noqa: F401
from . import gail  # noqa: F401
