"""TEST-ONLY stand-in for the `lightfm` package: polara/recommender/coldstart/models.py imports the reference's LightFM
wrapper unconditionally, and that wrapper imports this name.  Nothing here is ever instantiated."""


class LightFM:
    pass
