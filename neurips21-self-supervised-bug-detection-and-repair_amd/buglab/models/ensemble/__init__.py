"""Model ensembles (reference buglab/models/ensemble/): `wrapper.EnsembleWrapper` / `wrapper.EnsembleModuleWrapper`, and
`python -m buglab.models.ensemble OUT KIND MODEL...` to build an ensemble file that evaluate.py loads like any checkpoint.
Beyond the reference: the kind `weighted` (`_weights.EnsembleWeights`, `fit.fit_ensemble_weights`, `--fit-on VALID_DATA`)."""
