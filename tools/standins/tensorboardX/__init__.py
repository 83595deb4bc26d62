"""Stand-in for tensorboardX (authoring container only): train_next.py imports SummaryWriter at module level; the fixture
generator never logs."""


class SummaryWriter:
    def __init__(self, *args, **kwargs):
        pass

    def add_scalar(self, *args, **kwargs):
        pass

    def close(self):
        pass
