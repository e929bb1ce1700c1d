from .abstract import FeatureSieve
from .segment import *
from .increment import *
from .wrapper import *
from .implicit import *
