from audiolab_amd.wrappers.compare import Compare  # noqa: F401
from audiolab_amd.wrappers.remaster import Remaster  # noqa: F401
from audiolab_amd.wrappers.export import Export  # noqa: F401
