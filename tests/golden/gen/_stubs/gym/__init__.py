"""Stand-in for `gym`, just enough for `import linnaeus.rl_env.environment` to succeed in the golden generators: the environment
class is declared on top of gym.Env and builds gym.spaces objects in its constructor, which the generators never call."""


class Env:
    metadata = {}

    def reset(self, *, seed=None, options=None):
        return None


class _Space:
    def __init__(self, *args, **kwargs):
        self.args, self.kwargs = args, kwargs


class spaces:  # noqa: N801  (the module name the environment uses)
    Box = Discrete = MultiDiscrete = Dict = _Space
