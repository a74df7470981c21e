"""Import shim: lets the reference's import lines (``from src.fm import
FactorizationMachines``) resolve to the MI355X implementation when this
repository precedes the reference on ``sys.path``.  The drivers themselves
put their own directory first; run them with
``python -m relevance_factorizationmachine_amd.run``."""
