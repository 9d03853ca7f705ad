from .dataloaders_AtomTuple import (AtomTupleExtractor, BatchAtomTuple, Data,  # noqa: F401
                                    DataLoaderAtomTuple)
from .dataloaders_AtomTriple import (AtomTripleExtractor, BatchAtomTriple,  # noqa: F401
                                     DataLoaderAtomTriple)
from .device_dataset import DatasetBatch, DeviceDataset, DeviceLoader  # noqa: F401
