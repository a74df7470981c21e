from relevance_factorizationmachine_amd.optimizer import DeviceAdaGrad as AdaGrad  # noqa: F401
from relevance_factorizationmachine_amd.optimizer import DeviceSGD as SGD  # noqa: F401
