from .dataloaders_AtomTuple import (AtomTupleExtractor, BatchAtomTuple, Data,  # noqa: F401
                                    DataLoaderAtomTuple)
from .dataloaders_AtomTriple import (AtomTripleExtractor, BatchAtomTriple,  # noqa: F401
                                     DataLoaderAtomTriple)
from .dataloaders_LEP import BatchLEP, DataLoaderLEP  # noqa: F401
from .device_dataset import (DatasetBatch, DeviceDataset, DeviceLoader, PairedBatch,  # noqa: F401
                             PairedDeviceDataset)
