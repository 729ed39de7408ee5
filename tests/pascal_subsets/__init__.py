"""Tests of PASCAL groundtruth subsets: records, the host evaluator and the device labelling (mtlssl_pascal_match)."""
